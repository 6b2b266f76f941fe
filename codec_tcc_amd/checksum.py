"""CRC-32 checksums of covers and payloads (include/codec_tcc_crc.h): what MED-PEE decode
verifies, so that a stego, record or location map that is not what was embedded raises
IntegrityError instead of decoding to garbage.

CRC-32 as zlib computes it (reflected 0xEDB88320, init and final xor 0xFFFFFFFF):
  cover checksum of a slice   = zlib.crc32 of its pixels, row-major, little-endian bytes;
  payload checksum of a slice = zlib.crc32 of its L bits packed LSB-first into ceil(L / 8)
                                bytes, pad bits zero (framing.pack_bits' packing).

The cover checksum is one read-only streaming HIP pass on the caller's stream
(codec_crc32_slices); there is no CPU fallback.  CRC-32 detects corruption and
inconsistency, not an adversary.

Tile checksums (include/codec_tcc_tile.h) say WHERE a restored cover differs: one
CRC-32 per (th, tw) tile of every slice (crc32_tiles), two tables compared on the device
(compare_tiles); tiles_host is the same table from zlib.
"""
from __future__ import annotations

import ctypes as C
import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib
from .codec import _require_gpu, _stream, _torch


class IntegrityError(ValueError):
    """A decoded cover or payload does not have the checksum recorded at embed time.
    bad_cover / bad_payload: the slices whose cover / payload checksum failed.  tiles: when the
    encoding carried a tile table, {slice: bool ndarray [nty, ntx]} of the tiles of each
    bad_cover slice whose restored pixels differ ({} when no cover failed), else None.
    tile: the table's (th, tw), or None.
    keyed: True when a keyed embedding's Poly1305 tag failed (decode(key=)); slices then names the
    slices whose tag differs (their plaintext was zeroed on the device).
    rows: the payload rows exactly as the decode's one read-back brought them to the host (a
    volume: the stream's words; the failed slices of a keyed failure: the zeros the device
    released), None when the error was raised before any read-back."""

    def __init__(self, message="", *, bad_cover=(), bad_payload=(), tiles=None, tile=None, slices=(), keyed=False,
                 stream=False, rows=None):
        super().__init__(message)
        self.rows = rows
        self.slices = [int(b) for b in slices]
        self.keyed = bool(keyed)
        self.stream = bool(stream)   # a keyed volume: the stream's tag failed
        self.bad_cover = [int(b) for b in bad_cover]
        self.bad_payload = [int(b) for b in bad_payload]
        self.tiles = tiles
        self.tile = None if tile is None else (int(tile[0]), int(tile[1]))


def chunk_bytes() -> int:
    """Bytes of one slice one workgroup of the kernel covers (codec_crc32_chunk_bytes)."""
    return int(_lib.load().codec_crc32_chunk_bytes())


def crc32_slices(images, out=None):
    """CRC-32 of every slice of a [B,H,W] (or [H,W]) uint8 / uint16 GPU tensor: an int32 device
    tensor of B words holding the checksums' 32 bits (crc_list() gives them as Python ints).
    Asynchronous on the current stream, capturable; `out` (int32 [B], same device) is written
    when given.  ValueError for a non-contiguous tensor or another dtype; any byte alignment
    of the tensor's storage offset is exact."""
    _require_gpu()
    torch = _torch()
    if not isinstance(images, torch.Tensor):
        raise ValueError("crc32_slices takes a torch tensor on the GPU")
    if images.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"crc32_slices takes uint8 or uint16 pixels, got {images.dtype}")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or min(images.shape) < 1:
        raise ValueError("crc32_slices takes a [B,H,W] or [H,W] tensor with no empty dimension")
    if not images.is_cuda:
        raise ValueError("crc32_slices takes a tensor on the GPU")
    if not images.is_contiguous():
        raise ValueError("crc32_slices takes a contiguous tensor (the checksum is of the bytes as they lie)")
    B, H, W = (int(v) for v in images.shape)
    nbytes = images.element_size()
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=images.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B,) or not out.is_contiguous() or out.device != images.device:
        raise ValueError(f"out must be a contiguous int32 [{B}] tensor on the images' device")
    lib = _lib.load()
    ws = int(lib.codec_crc32_workspace_bytes(B, H, W, nbytes))
    if ws == 0:
        raise ValueError(f"crc32_slices: a batch of {B} x {H} x {W} is beyond the kernel's limits")
    work = torch.empty(ws, dtype=torch.uint8, device=images.device)
    _lib.check(lib.codec_crc32_slices(B, H, W, nbytes, images.data_ptr(), out.data_ptr(), work.data_ptr(), ws,
                                      _stream()), "codec_crc32_slices")
    return out


def crc_list(t) -> List[int]:
    """The checksums of a crc32_slices() tensor as unsigned Python ints (one read-back)."""
    return [int(v) & 0xFFFFFFFF for v in t.detach().cpu().tolist()]


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """CRC-32 of A || B from a = CRC-32(A), b = CRC-32(B) and B's length in bytes (pure host,
    the library's GF(2) routine: codec_crc32_combine)."""
    if len_b < 0:
        raise ValueError("len_b must be >= 0")
    out = C.c_uint32(0)
    _lib.check(_lib.load().codec_crc32_combine(int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF, int(len_b), C.byref(out)),
               "codec_crc32_combine")
    return int(out.value)


def payload_crc32(bits) -> int:
    """Payload checksum of one slice's 0/1 bit vector (host only)."""
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1)
    return zlib.crc32(np.packbits(bits, bitorder="little").tobytes()) & 0xFFFFFFFF


def payload_crc32_packed(words: np.ndarray, nbits: int) -> int:
    """payload_crc32 of the first nbits bits of one row of framing.pack_bits' packing (or of an
    extract's payload row) without unpacking it; bits past nbits in the last byte are ignored."""
    raw = np.ascontiguousarray(words).view(np.uint8).reshape(-1)
    nbits = int(nbits)
    nb = (nbits + 7) // 8
    if nb > raw.size:
        raise ValueError(f"{nbits} bits do not fit the row's {raw.size} bytes")
    if nbits % 8 == 0:
        return zlib.crc32(raw[:nb].tobytes()) & 0xFFFFFFFF
    last = bytes([int(raw[nb - 1]) & ((1 << (nbits % 8)) - 1)])
    return zlib.crc32(last, zlib.crc32(raw[:nb - 1].tobytes())) & 0xFFFFFFFF


def cover_crc32_host(image: np.ndarray) -> int:
    """The cover checksum of one slice computed on the host (zlib): what crc32_slices gives."""
    a = np.ascontiguousarray(image)
    return zlib.crc32(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()) & 0xFFFFFFFF


def verify_mode(verify) -> Optional[str]:
    """Normalise decode's `verify`: False -> None, True -> 'present', 'require' -> 'require'."""
    if verify is False:
        return None
    if verify is True:
        return "present"
    if verify == "require":
        return "require"
    raise ValueError("verify must be True, False or 'require'")


def raise_mismatch(bad_cover, bad_payload, what: str = "MED-PEE decode", *, tiles=None, tile=None, shape=None,
                   stream: bool = False, rows=None):
    """IntegrityError naming the slices whose cover / payload checksum failed (none: returns).
    tiles / tile: the differing-tile maps of the bad covers and their tile size (IntegrityError's
    attributes); shape = (H, W) lets the message give the tiles' pixel boxes.  stream: a volume's
    one payload checksum failed; rows: IntegrityError.rows."""
    if not bad_cover and not bad_payload and not stream:
        return
    parts = []
    if bad_cover:
        parts.append(f"cover checksum mismatch in slices {list(bad_cover)}")
    if bad_payload:
        parts.append(f"payload checksum mismatch in slices {list(bad_payload)}")
    if stream:
        parts.append("the volume's payload checksum does not match")
    raise IntegrityError(f"{what}: {'; '.join(parts)} (CRC-32: this is not what was embedded)"
                         + tiles_text(tiles, tile, shape),
                         bad_cover=bad_cover, bad_payload=bad_payload, tiles=tiles, tile=tile, rows=rows)


# ------------------------------------------------------------------ tile checksums
TILE_DEFAULT = 64
_TILES_SHOWN = 4   # differing tiles an IntegrityError message lists per slice


def check_tile_args(tile) -> Tuple[int, int]:
    """(th, tw) of a `tile` argument: an int (square) or a pair of ints, each 4..1024
    (include/codec_tcc_tile.h).  ValueError otherwise.  Pure host code: no GPU, no library load."""
    t = (tile, tile) if not isinstance(tile, (tuple, list)) else tuple(tile)
    if len(t) != 2:
        raise ValueError(f"tile must be an int or a (th, tw) pair, got {tile!r}")
    out = []
    for v in t:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"tile sizes are integers in {_lib.TILE_MIN}..{_lib.TILE_MAX}, got {tile!r}")
        if not _lib.TILE_MIN <= int(v) <= _lib.TILE_MAX:
            raise ValueError(f"tile sizes are integers in {_lib.TILE_MIN}..{_lib.TILE_MAX}, got {tile!r}")
        out.append(int(v))
    return out[0], out[1]


def checksum_mode(checksum) -> Tuple[bool, bool]:
    """(slice checksums, tile checksums) of embed's `checksum`: False, True or "tiles" (any other
    string is a ValueError; other values count by their truth, as they always did)."""
    if isinstance(checksum, str):
        if checksum != "tiles":
            raise ValueError("checksum must be True, False or 'tiles'")
        return True, True
    return bool(checksum), False


def tile_grid(H: int, W: int, tile=TILE_DEFAULT) -> Tuple[int, int]:
    """(nty, ntx) = (ceil(H / th), ceil(W / tw)): the tile table's grid (pure host)."""
    th, tw = check_tile_args(tile)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"tile_grid takes a slice of at least 1 x 1 pixels, got {H} x {W}")
    return -(-H // th), -(-W // tw)


def tiles_host(image: np.ndarray, tile=TILE_DEFAULT) -> np.ndarray:
    """The tile table of one [H, W] uint8 / uint16 slice computed on the host (zlib): uint32
    [nty, ntx], what crc32_tiles gives for the slice."""
    a = np.asarray(image)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.uint16):
        raise ValueError("tiles_host takes one [H, W] uint8 or uint16 slice")
    th, tw = check_tile_args(tile)
    nty, ntx = tile_grid(a.shape[0], a.shape[1], (th, tw))
    out = np.empty((nty, ntx), dtype=np.uint32)
    for i in range(nty):
        for j in range(ntx):
            out[i, j] = cover_crc32_host(a[i * th:(i + 1) * th, j * tw:(j + 1) * tw])
    return out


def _gpu_batch(images, what: str):
    torch = _torch()
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{what} takes a torch tensor on the GPU")
    if images.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"{what} takes uint8 or uint16 pixels, got {images.dtype}")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or min(images.shape) < 1:
        raise ValueError(f"{what} takes a [B,H,W] or [H,W] tensor with no empty dimension")
    if not images.is_cuda:
        raise ValueError(f"{what} takes a tensor on the GPU")
    if not images.is_contiguous():
        raise ValueError(f"{what} takes a contiguous tensor (the checksum is of the bytes as they lie)")
    return images


def crc32_tiles(images, tile=TILE_DEFAULT, out=None):
    """CRC-32 of every (th, tw) tile of every slice of a [B,H,W] (or [H,W]) uint8 / uint16 GPU
    tensor: an int32 device tensor [B, nty, ntx] holding the checksums' 32 bits (tiles_host gives
    the same table from zlib).  One launch on the current stream, capturable, no workspace; `out`
    (int32 [B, nty, ntx], same device) is written when given.  Arguments as crc32_slices; any byte
    alignment of the storage offset is exact (16-byte-aligned layouts take the vector kernel)."""
    th, tw = check_tile_args(tile)
    _require_gpu()
    torch = _torch()
    images = _gpu_batch(images, "crc32_tiles")
    B, H, W = (int(v) for v in images.shape)
    nty, ntx = tile_grid(H, W, (th, tw))
    if out is None:
        out = torch.empty((B, nty, ntx), dtype=torch.int32, device=images.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, nty, ntx) or not out.is_contiguous() or \
            out.device != images.device:
        raise ValueError(f"out must be a contiguous int32 [{B}, {nty}, {ntx}] tensor on the images' device")
    _lib.check(_lib.load().codec_crc32_tiles(B, H, W, images.element_size(), th, tw, images.data_ptr(), out.data_ptr(),
                                             _stream()), "codec_crc32_tiles")
    return out


def tiles_route(images, tile=TILE_DEFAULT) -> int:
    """The route mask of crc32_tiles(images, tile) (codec_crc32_tiles_route: 1 = byte route,
    2 = vector route); looks at the tensor's shape and address only."""
    th, tw = check_tile_args(tile)
    images = images if images.dim() == 3 else images[None]
    B, H, W = (int(v) for v in images.shape)
    rc = int(_lib.load().codec_crc32_tiles_route(B, H, W, images.element_size(), th, tw, images.data_ptr()))
    if rc < 0:
        _lib.check(rc, "codec_crc32_tiles_route")
    return rc


def compare_tiles(got, want, out=None):
    """(count, bitmap) of two tile tables of one shape [B, ...] (int32, same device): count
    int32 [B] = tiles of slice b that differ, bitmap int64 [B, ceil(nt / 64)] with bit t % 64 of
    word t // 64 set when tile t (row-major) differs, bits past nt zero.  One launch on the
    current stream, capturable; out = (count, bitmap) is written when given."""
    _require_gpu()
    torch = _torch()
    for t in (got, want):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() < 2 or not t.is_contiguous() \
                or not t.is_cuda:
            raise ValueError("compare_tiles takes two contiguous int32 tile tables [B, ...] on the GPU")
    if got.shape != want.shape or got.device != want.device or got.numel() == 0:
        raise ValueError(f"compare_tiles takes two non-empty tables of one shape and device, got {tuple(got.shape)} on "
                         f"{got.device} and {tuple(want.shape)} on {want.device}")
    B = int(got.shape[0])
    nt = got.numel() // B
    nw = (nt + 63) // 64
    if out is None:
        count = torch.empty(B, dtype=torch.int32, device=got.device)
        bitmap = torch.empty((B, nw), dtype=torch.int64, device=got.device)
    else:
        count, bitmap = out
        if count.dtype != torch.int32 or tuple(count.shape) != (B,) or bitmap.dtype != torch.int64 or \
                tuple(bitmap.shape) != (B, nw) or not (count.is_contiguous() and bitmap.is_contiguous()) or \
                count.device != got.device or bitmap.device != got.device:
            raise ValueError(f"out must be (int32 [{B}], int64 [{B}, {nw}]) contiguous tensors on the tables' device")
    _lib.check(_lib.load().codec_crc32_tiles_compare(B, nt, got.data_ptr(), want.data_ptr(), bitmap.data_ptr(),
                                                     count.data_ptr(), _stream()), "codec_crc32_tiles_compare")
    return count, bitmap


def bitmap_mask(words: np.ndarray, nty: int, ntx: int) -> np.ndarray:
    """One slice's row of compare_tiles' bitmap (host) as a bool [nty, ntx] map."""
    raw = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[: nty * ntx].astype(bool).reshape(nty, ntx)


def check_tile_table(table, B: int, H: int, W: int, tile, device=None) -> Tuple[int, int]:
    """(nty, ntx) when `table` is the int32 [B, nty, ntx] table of B slices of H x W at `tile`
    (on `device` when given); ValueError for another grid, dtype or device."""
    torch = _torch()
    nty, ntx = tile_grid(H, W, tile)
    if not isinstance(table, torch.Tensor):
        raise ValueError("a tile table is an int32 torch tensor [B, nty, ntx]")
    if table.dtype != torch.int32:
        raise ValueError(f"a tile table is int32, got {table.dtype}")
    if tuple(table.shape) != (B, nty, ntx):
        raise ValueError(f"a tile table of shape {tuple(table.shape)} for {B} slices of {H} x {W} at tile "
                         f"{tuple(check_tile_args(tile))}: [{B}, {nty}, {ntx}] expected")
    if device is not None and table.device != device:
        raise ValueError(f"the tile table lies on {table.device}, the pixels on {device}")
    if not table.is_contiguous():
        raise ValueError("a tile table must be contiguous")
    return nty, ntx


def tile_mismatch_maps(cover, table, tile, slices=None) -> Dict[int, np.ndarray]:
    """{slice: bool [nty, ntx]} of the tiles of `cover` ([B,H,W] on the GPU) whose CRC-32 differs
    from `table`'s (int32 [B, nty, ntx] on the same device): crc32_tiles + compare_tiles on the
    current stream, then one read-back of counts and bitmap (never of the tables).  slices: the
    slices to report (default: those with a differing tile)."""
    torch = _torch()
    cover = _gpu_batch(cover, "tile_mismatch_maps")
    B, H, W = (int(v) for v in cover.shape)
    nty, ntx = check_tile_table(table, B, H, W, tile, cover.device)
    count, bitmap = compare_tiles(crc32_tiles(cover, tile), table)
    host = torch.cat([bitmap.reshape(-1), count.to(torch.int64)]).cpu().numpy()
    words, counts = host[:-B].reshape(B, -1), host[-B:]
    which = [b for b in range(B) if counts[b]] if slices is None else [int(b) for b in slices]
    return {b: bitmap_mask(words[b], nty, ntx) for b in which}


def tile_box(i: int, j: int, tile, shape) -> Tuple[int, int, int, int]:
    """(r0, r1, c0, c1): tile (i, j) covers rows [r0, r1) and columns [c0, c1) of an H x W slice."""
    th, tw = tile
    return i * th, min(int(shape[0]), (i + 1) * th), j * tw, min(int(shape[1]), (j + 1) * tw)


def tiles_text(tiles, tile, shape=None) -> str:
    """The tail an IntegrityError message gains when tile maps are present: the first few
    differing tiles of each slice as (row, column), with their pixel boxes when shape is known."""
    if not tiles:
        return ""
    parts = []
    for b in sorted(tiles):
        ij = np.argwhere(tiles[b])
        shown = []
        for i, j in ij[:_TILES_SHOWN]:
            txt = f"({int(i)}, {int(j)})"
            if shape is not None and tile is not None:
                r0, r1, c0, c1 = tile_box(int(i), int(j), tile, shape)
                txt += f" = rows {r0}..{r1 - 1}, columns {c0}..{c1 - 1}"
            shown.append(txt)
        more = f" and {len(ij) - _TILES_SHOWN} more" if len(ij) > _TILES_SHOWN else ""
        parts.append(f"slice {b}: {len(ij)} of {tiles[b].size} tiles differ" +
                     (f", (row, column) {'; '.join(shown)}{more}" if shown else ""))
    head = "; tiles: " if tile is None else f"; tiles of {tile[0]} x {tile[1]}: "
    return head + " | ".join(parts)

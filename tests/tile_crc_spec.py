"""The tile checksums' definition as plain host code (include/codec_tcc_tile.h): zlib
is the oracle, nothing here touches the package's own routines.

Tile size (th, tw), integers in 4..1024 (a single int: square).  nty = ceil(H / th),
ntx = ceil(W / tw).  Tile (i, j) covers rows [i th, min(H, (i + 1) th)) and columns
[j tw, min(W, (j + 1) tw)); its checksum is zlib's CRC-32 of those pixels, row-major inside the
tile, as little-endian bytes.  A table is [B, nty, ntx]."""
import zlib

import numpy as np

TILE_MIN, TILE_MAX = 4, 1024


def tile_pair(tile):
    th, tw = (tile, tile) if isinstance(tile, (int, np.integer)) else tile
    th, tw = int(th), int(tw)
    if not (TILE_MIN <= th <= TILE_MAX and TILE_MIN <= tw <= TILE_MAX):
        raise ValueError(f"tile {tile!r} outside {TILE_MIN}..{TILE_MAX}")
    return th, tw


def grid(H: int, W: int, tile):
    th, tw = tile_pair(tile)
    return (H + th - 1) // th, (W + tw - 1) // tw


def box(i: int, j: int, H: int, W: int, tile):
    """(r0, r1, c0, c1) of tile (i, j)."""
    th, tw = tile_pair(tile)
    return i * th, min(H, (i + 1) * th), j * tw, min(W, (j + 1) * tw)


def tile_table(img: np.ndarray, tile) -> np.ndarray:
    """uint32 [nty, ntx] of one [H, W] uint8 / uint16 slice, or [B, nty, ntx] of a [B, H, W] stack."""
    img = np.asarray(img)
    if img.ndim == 3:
        return np.stack([tile_table(s, tile) for s in img])
    assert img.ndim == 2 and img.dtype in (np.uint8, np.uint16)
    H, W = img.shape
    nty, ntx = grid(H, W, tile)
    le = "<u2" if img.dtype == np.uint16 else "u1"
    out = np.empty((nty, ntx), dtype=np.uint32)
    for i in range(nty):
        for j in range(ntx):
            r0, r1, c0, c1 = box(i, j, H, W, tile)
            out[i, j] = zlib.crc32(img[r0:r1, c0:c1].astype(le).tobytes()) & 0xFFFFFFFF
    return out


def mismatch_map(a: np.ndarray, b: np.ndarray, tile) -> np.ndarray:
    """bool [nty, ntx] (or [B, nty, ntx]): the tiles in which two images of one shape differ in
    any pixel -- what comparing their tile tables reports, CRC collisions aside."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    if a.ndim == 3:
        return np.stack([mismatch_map(x, y, tile) for x, y in zip(a, b)])
    H, W = a.shape
    nty, ntx = grid(H, W, tile)
    out = np.zeros((nty, ntx), dtype=bool)
    d = a != b
    for i in range(nty):
        for j in range(ntx):
            r0, r1, c0, c1 = box(i, j, H, W, tile)
            out[i, j] = bool(d[r0:r1, c0:c1].any())
    return out


def bitmap_words(mask: np.ndarray) -> np.ndarray:
    """uint64 [ceil(nt / 64)]: bit t % 64 of word t // 64 = tile t (row-major) of `mask`, pad bits zero."""
    flat = np.asarray(mask, dtype=bool).reshape(-1)
    pad = np.zeros((flat.size + 63) // 64 * 64, dtype=np.uint8)
    pad[: flat.size] = flat
    return np.packbits(pad, bitorder="little").view("<u8").astype(np.uint64)

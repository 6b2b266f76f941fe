/*
 * codec_tcc_tile.h -- tile checksums of libcodec_hip.so: one CRC-32 per 2-D tile of every slice,
 * so that MED-PEE verify can say WHICH tiles of a restored cover are not what was embedded
 * (DESIGN section 3h).  Same boundary contract as codec_tcc.h (device pointers, asynchronous on
 * `stream`, 0 or a negative status with a codec_last_error text, no allocation, capture-safe).
 *
 * Definition (tests/tile_crc_spec.py is the executable form, zlib the oracle).  A tile size is
 * (th, tw), each CODEC_TILE_MIN .. CODEC_TILE_MAX.  nty = ceil(H / th), ntx = ceil(W / tw).  Tile
 * (i, j) covers rows [i th, min(H, (i + 1) th)) and columns [j tw, min(W, (j + 1) tw)); edge
 * tiles are simply smaller.  Its checksum is CRC-32 (codec_tcc_crc.h's: zlib's) of those pixels,
 * row-major inside the tile, as little-endian bytes.  A table is uint32 [B, nty, ntx].
 *
 * Routes.  A call takes ONE route for all its tiles:
 *   vector route -- when tw * bytes, W * bytes and the address `images` are multiples of 16 (every
 *                   tile row, the last column's included, is then a whole number of aligned 16-B
 *                   vectors): one wave per tile, four waves sharing the tables of a (slice, tile
 *                   row) band;
 *   byte route   -- everything else (odd widths, tile rows that are no multiple of 16 B, storage
 *                   of any byte alignment): one lane per tile row, bytewise.  Exact, not fast.
 * A mixed call does not exist: the vector route's conditions make the last column's rows whole
 * vectors too.  codec_crc32_tiles_route tells which route a call takes.
 */
#ifndef CODEC_TCC_TILE_H
#define CODEC_TCC_TILE_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_TILE_CRC 43       /* vector route: one wave per tile                      */
#define CODEC_K_TILE_CRC_BYTES 44 /* byte route: one lane per tile row                    */
#define CODEC_K_TILE_COMPARE 45   /* two tables -> differing-tile bitmap and counts       */

#define CODEC_TILE_MIN 4
#define CODEC_TILE_MAX 1024

#define CODEC_TILE_ROUTE_BYTES 1  /* codec_crc32_tiles_route: some tile takes the byte route   */
#define CODEC_TILE_ROUTE_VECTOR 2 /* ... some tile takes the vector route                      */

/* Pure host: *nty = ceil(H / th), *ntx = ceil(W / tw).  Negative for H or W < 1, a tile size
 * outside CODEC_TILE_MIN .. CODEC_TILE_MAX, H * W > 2^31 or a NULL pointer. */
int codec_crc32_tiles_grid(int32_t H, int32_t W, int32_t th, int32_t tw, int32_t* nty, int32_t* ntx);

/* Pure host: the routes codec_crc32_tiles takes for these arguments, as a mask of
 * CODEC_TILE_ROUTE_*.  This build returns exactly one bit (see "Routes" above); `images` is
 * looked at for its alignment only.  Negative for arguments codec_crc32_tiles refuses. */
int codec_crc32_tiles_route(int32_t B, int32_t H, int32_t W, int32_t bytes, int32_t th, int32_t tw,
                            const void* images);

/* crc[(b * nty + i) * ntx + j] (device uint32) = CRC-32 of tile (i, j) of slice b, the slices
 * being the B contiguous [H, W] images of `bytes` = 1 or 2 bytes per pixel at `images`.
 * Read-only on `images`; one launch on `stream`; no workspace.  Refused: B, H or W < 1, bytes
 * other than 1 or 2, a tile size out of range, H * W > 2^31, B * nty * ntx >= 2^31, NULL. */
int codec_crc32_tiles(int32_t B, int32_t H, int32_t W, int32_t bytes, int32_t th, int32_t tw, const void* images,
                      uint32_t* crc, void* stream);

/* Two tables [B, nt] (device uint32) -> count[b] (device int32) = tiles of slice b that differ,
 * bitmap[b * ceil(nt / 64) + t / 64] (device uint64) bit t % 64 = tile t of slice b differs;
 * bits past nt are zero.  Every word of both outputs is written.  One launch on `stream`.
 * Refused: B or nt < 1, B * nt >= 2^31, NULL. */
int codec_crc32_tiles_compare(int32_t B, int32_t nt, const uint32_t* got, const uint32_t* want, uint64_t* bitmap,
                              int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_TILE_H */

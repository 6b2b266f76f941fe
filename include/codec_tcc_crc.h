/*
 * codec_tcc_crc.h -- CRC-32 entries of libcodec_hip.so (the checksums MED-PEE decode verifies).
 * Same boundary contract as codec_tcc.h (device pointers, asynchronous on `stream`, 0 or a
 * negative status with a codec_last_error text).
 *
 * CRC-32 as zlib, PNG and DICOM-deflate compute it: reflected polynomial 0xEDB88320, initial
 * value and final xor 0xFFFFFFFF.  A slice's checksum is that of its pixels in row-major order
 * as little-endian bytes, i.e. of its H * W * bytes bytes as they lie in memory.
 */
#ifndef CODEC_TCC_CRC_H
#define CODEC_TCC_CRC_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_CRC32 36         /* streaming pass: one raw partial per chunk          */
#define CODEC_K_CRC32_COMBINE 37 /* chunk partials -> one checksum per slice           */

/* Bytes of one slice one workgroup covers (slices are cut into chunks of this size from their
 * first byte; the last chunk is the remainder). */
size_t codec_crc32_chunk_bytes(void);

/* Workspace of codec_crc32_slices (one 32-bit partial per chunk); 0 for bad arguments.  The
 * call keeps no state in it. */
size_t codec_crc32_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t bytes);

/* crc[b] (device uint32, b < B) = CRC-32 of slice b: the H * W * bytes bytes at
 * images + b * H * W * bytes.  bytes = 1 or 2; no alignment is required of `images` (slice
 * bases of any byte alignment are exact).  Read-only on `images`; two launches on `stream`, no
 * host synchronisation, no allocation, capture-safe. */
int codec_crc32_slices(int32_t B, int32_t H, int32_t W, int32_t bytes, const void* images, uint32_t* crc,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Pure host: *out = CRC-32 of A || B given crc_a = CRC-32(A), crc_b = CRC-32(B) and B's length
 * in bytes -- crc_a * x^(8 len_b) + crc_b over GF(2) modulo the polynomial, by the routine the
 * kernel's constants are made with. */
int codec_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_CRC_H */

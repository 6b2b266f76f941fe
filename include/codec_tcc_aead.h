/*
 * codec_tcc_aead.h -- keyed MED-PEE: ChaCha20-Poly1305 (RFC 8439) over payload rows and covers,
 * entries of libcodec_hip.so.  Same boundary contract as codec_tcc.h: device pointers, a
 * caller-provided workspace, asynchronous on `stream`, no allocation, no host synchronisation,
 * capturable; 0 or a negative status with a codec_last_error text.  Arguments are checked in the
 * order each entry documents, before any device operation.
 *
 * Construction (the specification is tests/aead_spec.py).  Slice b of a call has the
 * global index g = index0 + b.
 *   nonce12 = LE32(g) || nonce (8 bytes)
 *   otk     = ChaCha20(key, counter 0, nonce12)[0:32], r clamped and s taken as RFC 8439 §2.5
 *   CT      = PT xor keystream(counter 1, 2, ...) on the first L bits of the row; bit i of a row
 *             is bit i % 64 of 64-bit word i / 64 (keystream byte k meets bits 8k .. 8k+7); bits
 *             at and past L are 0
 *   nb      = ceil(L / 8)
 *   tag     = Poly1305(otk, pad16(AAD) || pad16(CT[0:nb]) || LE64(len AAD) || LE64(nb))
 * For L % 8 == 0 this is RFC 8439 §2.8.  Per-slice indices are < 2^31; 0x80000000
 * (CODEC_AEAD_STREAM_INDEX) is reserved for a volume's stream, a call of B = 1.  A row holds at
 * most 2^31 - 1 bits, so the 32-bit block counter never wraps.
 *
 * Rows are arrays of uint64 words, [B][row_words], 8-byte aligned.  `lengths` (device int32 [B])
 * holds each row's L in bits; a value outside 0 .. 64 * row_words counts as the nearer bound.
 */
#ifndef CODEC_TCC_AEAD_H
#define CODEC_TCC_AEAD_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_CHACHA20_ROWS 47   /* keystream xor over (row, 64-byte block) pairs          */
#define CODEC_K_POLY1305_PREP 48   /* one-time key and power table of every slice             */
#define CODEC_K_POLY1305 49        /* streaming pass over the AAD: one partial per chunk      */
#define CODEC_K_POLY1305_FINISH 50 /* partials, CT blocks, lengths block, final reduction     */
#define CODEC_K_AEAD_RELEASE 51    /* tag comparison and decryption                           */

#define CODEC_AEAD_STREAM_INDEX 0x80000000u
#define CODEC_AEAD_MAX_ROW_WORDS (1 << 25)   /* the words that hold 2^31 - 1 bits (lengths are int32) */

/* Key and nonce of a call.  The block lives in DEVICE memory: key and nonce never enter a
 * kernel's argument list, and a captured graph is replayed under a fresh nonce by rewriting
 * the block between replays.  Replaying a captured graph WITHOUT rewriting it reuses the nonce,
 * which voids both the confidentiality and the authentication of the construction. */
typedef struct codec_aead_ctx {
    uint32_t key[8];      /* the 32 key bytes as little-endian words   */
    uint32_t nonce[2];    /* the 8 nonce bytes as little-endian words  */
    uint32_t reserved[2]; /* 0 */
} codec_aead_ctx;         /* 48 bytes */

/* Bytes of one slice's AAD one workgroup of the streaming pass covers (a multiple of 16). */
size_t codec_poly1305_chunk_bytes(void);

/* Workspace of the tag calls for B slices of aad_bytes bytes of AAD and rows of row_words words
 * (0 for a call without rows); 0 for bad arguments.  No state survives a call. */
size_t codec_aead_workspace_bytes(int32_t B, int64_t aad_bytes, int32_t row_words);

/* rows_out[b] = rows_in[b] xor the keystream of slice index0 + b on its first lengths[b] bits,
 * zero past them; every word of rows_out is written.  rows_out may be rows_in.  One launch.
 * Checks: B >= 1; 1 <= row_words <= CODEC_AEAD_MAX_ROW_WORDS and the batch within the grid
 * limit; the indices (above); NULL pointers. */
int codec_chacha20_rows(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint64_t* rows_in,
                        int32_t row_words, const int32_t* lengths, uint64_t* rows_out, void* stream);

/* tags[b][0..3] (device uint32, the tag's 16 bytes as little-endian words) of slice index0 + b:
 * AAD = the aad_bytes bytes at aad + b * aad_bytes (any byte alignment is exact; 16-byte-aligned
 * slice bases take the vector loads), CT = the first lengths[b] bits of ct_rows[b].  aad may be
 * NULL with aad_bytes 0; ct_rows may be NULL with lengths NULL and row_words 0 (an empty CT).
 * Read-only on aad and ct_rows.  Two launches plus one when aad_bytes > 0.
 * Checks: B >= 1; aad_bytes >= 0 and aad NULL exactly when it is 0; row_words 0 with ct_rows and
 * lengths both NULL, else 1 .. CODEC_AEAD_MAX_ROW_WORDS with both given; the batch within the
 * grid limit; the indices; ctx / tags / workspace NULL; workspace_bytes. */
int codec_poly1305_tags(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const void* aad, int64_t aad_bytes,
                        const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths, uint32_t* tags,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The same pass with the one-time keys given (device uint32 [B][8]: r unclamped then s) instead
 * of derived; codec_poly1305_tags is "derive, then this".  Tests choose r and s with it. */
int codec_poly1305_tags_otk(const uint32_t* otk, int32_t B, const void* aad, int64_t aad_bytes,
                            const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths, uint32_t* tags,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ok[b] (device int32) = 1 iff all 128 bits of tags_got[b] and tags_want[b] agree -- the XOR of
 * the words is OR-reduced, with no early exit and no data-dependent branch; pt_rows_out[b] =
 * ct_rows[b] decrypted (as codec_chacha20_rows) when ok[b], else all zeros.  pt_rows_out may be
 * ct_rows.  One launch.  Checks: as codec_chacha20_rows, then the tag and ok pointers. */
int codec_aead_release(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint32_t* tags_got,
                       const uint32_t* tags_want, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                       uint64_t* pt_rows_out, int32_t* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_AEAD_H */

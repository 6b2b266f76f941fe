/*
 * codec_tcc_blind_keyed.h -- keyed blind MED-PEE: the stego carries its nonce and its Poly1305 tag,
 * so that a 32-byte key is all a reader needs besides the pixels.  The entries stand beside those
 * of codec_tcc_blind.h, codec_tcc_blind_auto.h and codec_tcc_aead.h and share their boundary
 * contract (device pointers, a caller-provided workspace, asynchronous on `stream`, no allocation,
 * no host synchronisation, capturable into a graph, 0 or a negative status with a
 * codec_last_error text).
 *
 * The format (specification: tests/pee_blind_keyed_spec.py) is codec_tcc_blind.h's with
 * flag bit 1 of header word 1 (CODEC_PEE_BLIND_FLAG_KEYED) set, flag bit 0 clear and word 5 = 0.
 * The user bits of such a slice are a 224-bit frame and the ciphertext:
 *   user stream = nonce12 (12 bytes) || tag (16 bytes) || CT (n_ct bits);  header n_user = 224 + n_ct
 * with nonce12 = LE32(g) || nonce, g = index0 + b, CT and tag as codec_tcc_aead.h defines them, the
 * AAD being the cover slice's bytes.  Byte k of the frame occupies user bits 8k .. 8k+7, LSB
 * first: as 64-bit row words, 0 = g | nonce[0] << 32, 1 = nonce[1] | tag[0] << 32, 2 = tag[1] |
 * tag[2] << 32, 3 = tag[3] | CT[0:32] << 32, and the ciphertext goes on, 32 bits off a word.  The
 * plan sees n_user = 224 + n_ct and is otherwise unchanged; nothing in the frame is secret.
 *
 * No kernel waits on another workgroup; what crosses launches goes through stream order.  Lengths,
 * header words, frame words and the chosen T are clamped to the rows, the slice and 1..64 wherever
 * a kernel reads them back from device memory.
 */
#ifndef CODEC_TCC_BLIND_KEYED_H
#define CODEC_TCC_BLIND_KEYED_H

#include "codec_tcc_aead.h"
#include "codec_tcc_blind_auto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_PEE_BLIND_FLAG_KEYED 2
#define CODEC_PEE_BLIND_FRAME_BITS 224
#define CODEC_PEE_BLIND_FRAME_WORDS 7 /* uint32 words of a frame: g, nonce[0..1], tag[0..3] */

/* ---- the AEAD entries of codec_tcc_aead.h with one nonce per slice.  nonce12: device uint32
 * [B][3] = (g, nonce word 0, nonce word 1) of slice b, used with ctx's key (ctx's own nonce words
 * are ignored).  No index rule applies: a decoder takes g from the stego, and a forged one only
 * makes the tag fail.  For nonce12[b] = (index0 + b, ctx's nonce) the results are the namesakes'
 * bit for bit.  Checks: the namesake's, without the indices and with nonce12 among the pointers. */
int codec_chacha20_rows_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const uint64_t* rows_in,
                          int32_t row_words, const int32_t* lengths, uint64_t* rows_out, void* stream);

int codec_poly1305_tags_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const void* aad,
                          int64_t aad_bytes, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                          uint32_t* tags, void* workspace, size_t workspace_bytes, void* stream);

int codec_aead_release_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const uint32_t* tags_got,
                         const uint32_t* tags_want, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                         uint64_t* pt_rows_out, int32_t* ok, void* stream);

/* frames_out: device uint32 [B][7] = (index0 + b, ctx->nonce[0], ctx->nonce[1], tags[b][0..3]).  The
 * nonce is read on the device from the ctx block, so a captured embed replays correctly after the
 * block is rewritten.  One launch.  Checks: B >= 1; the indices (codec_tcc_aead.h); NULL pointers. */
int codec_pee_blind_frames(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint32_t* tags,
                           uint32_t* frames_out, void* stream);

/* cover -> keyed stego, out of place.  frames: device uint32 [B][7] (codec_pee_blind_frames);
 * ct_rows: device [B][ct_words] uint64, the ciphertext rows; lengths: device int32 [B], n_ct in
 * bits (clamped to 0 .. 64 ct_words).  tmax == 0: the fixed P->T as codec_pee_blind_embed (ts is
 * not used and may be NULL); tmax in 1..16: T chosen per slice as codec_pee_blind_embed_auto does
 * (ts: device int32 [B], T* or 0; P->T is only range-checked).  The steps are the unkeyed ones --
 * row table, plan, splice, codec_pee_roi_embed, pack -- with n_user = 224 + n_ct, the user stream
 * frames[b] || ct_rows[b] (the splice reads through the frame: no shifted copy is made), flag bit
 * 1 set and no CRC.  P->payload_words >= CODEC_PEE_BLIND_ROW_WORDS(max n_ct + 224, max_entries):
 * a slice whose side and user bits exceed the row is refused with status 1.  info, meta, lm: as
 * codec_pee_blind_embed's; info[1] is the header's n_user, frame included.
 * Workspace: codec_pee_blind_workspace_bytes(P, max_entries) for tmax == 0, else
 * codec_pee_blind_auto_workspace_bytes(P, tmax, max_entries).
 * Checks, in this order, before any device operation: params NULL, max_entries, tmax in 0..16,
 * then codec_tcc_blind.h's list from the params' own ranges on (H, W <= 65535, T <= 64, H W >= 192,
 * the row width, which here includes the frame), NULL pointers (ts when tmax > 0), cover == stego,
 * ct_words in 1..2^24, the workspace size. */
int codec_pee_blind_embed_keyed(const codec_pee_params* P, const void* cover, void* stego, const uint32_t* frames,
                                const uint64_t* ct_rows, int32_t ct_words, const int32_t* lengths, int32_t tmax,
                                int32_t max_entries, int32_t* info, int32_t* ts, codec_pee_meta* meta, uint64_t* lm,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The user rows codec_pee_blind_extract wrote (rows: device [B][user_words] uint64) and the gathered
 * headers (hdr: device uint32 [B][8]) -> nonce12_out [B][3], tags_out [B][4] (device uint32; frame
 * words a row of fewer than four words lacks are 0), ct_out [B][ct_words] uint64 = the ciphertext
 * shifted down by 224 bits (whole rows are written; bits past n_ct are 0) and ct_lengths_out
 * (device int32 [B]) = clamp(min(hdr n_user, 64 user_words) - 224, 0, 64 ct_words).  One launch, no
 * workspace.  Checks: B in 1..65535; user_words and ct_words in 1..2^24; NULL pointers. */
int codec_pee_blind_unframe(int32_t B, const uint64_t* rows, int32_t user_words, const uint32_t* hdr,
                            uint32_t* nonce12_out, uint32_t* tags_out, uint64_t* ct_out, int32_t ct_words,
                            int32_t* ct_lengths_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_BLIND_KEYED_H */

/*
 * codec_tcc_blind_vol.h -- blind volume payloads: one bitstream planned on the device across a
 * stack of blind MED-PEE stegos (codec_tcc_blind.h, codec_tcc_blind_auto.h), each of which names its
 * place in the stream, so that the pixels alone decode it, in any slice order.  The entries share the
 * boundary contract of codec_tcc_blind.h (device pointers, a caller-provided workspace, asynchronous
 * on `stream`, no allocation, no host synchronisation, capturable into a graph, 0 or a negative
 * status with a codec_last_error text).  Specification: tests/pee_blind_volume_spec.py; DESIGN §3n.
 *
 * Format.  The blind format with flag bit 2 (CODEC_PEE_BLIND_FLAG_VOLUME) in header word 1: the
 * first 192 user bits are a frame of six 32-bit words, LSB first:
 *   0 volume_id (the caller's 32 bits)      3 off_b, the first stream bit the slice carries
 *   1 b, the slice's index in the stack     4 N, the stream's length in bits
 *   2 B (bits 0-15) | frame flags (16-31;   5 zlib CRC-32 of the stream's ceil(N / 8) bytes (pad
 *     bit 16: word 5 holds the CRC)           bits zero), or 0
 * and the share, stream bits [off_b, off_b + n_b), follows it: n_user = 192 + n_b.  Header flag bit 0
 * (cover CRC) keeps its meaning; bit 1 (keyed) is not combined with bit 2.
 *
 * Plan.  curve[b][T-1]: the blind capacity at T (codec_pee_blind_plan_auto); c[b][T-1] = curve - 192
 * where curve >= 192, else 0; S(T) = sum_b c[b][T-1]; T* the smallest T with S(T) >= N.  With
 * c_b = c[b][T*-1], P_b its exclusive prefix sum, P_B = S(T*):
 *   CODEC_VOL_EVEN (0)  off_b = floor(N P_b / P_B), n_b = floor(N P_(b+1) / P_B) - off_b
 *   CODEC_VOL_FILL (1)  off_b = min(N, P_b), n_b = min(c_b, N - off_b)
 * (codec_tcc_vol.h's rule).  S(tmax) < N: the volume is REFUSED, info status 1 -- every slice is
 * copied through and no header is written (a blind volume never truncates).  A slice with n_b = 0
 * is copied through without a header: per-slice info status CODEC_PEE_BLIND_SKIPPED, t_out 0.  A
 * carrier is embedded exactly as codec_pee_blind_embed_auto embeds the user stream frame || share,
 * with flag bit 2 set; its T is the smallest whose plan takes 192 + n_b bits.
 *
 * Plan info (device int32 [8]): status (0, or 1 refused), T*, S(T*), S(tmax), carriers, N, policy, B.
 *
 * Decode.  codec_pee_blind_headers, read back by the caller, who marks the slices without a header
 * in skip (device int32 [B], nonzero: no carrier) and builds the records (a skipped slice's record
 * copies through: L = 0, end = -1).  codec_pee_blind_volume_extract then runs the blind extract,
 * the order and the gather:
 *   order   one workgroup.  Carriers must agree on frame words 0, 2, 4 and 5; an index must be below
 *           the frame's B and distinct; off_b + n_b <= N.  Each carrier writes its index slot and
 *           reads it back after the barrier (a duplicate shows without atomics); offsets are
 *           monotone in the index, so the slots are the carriers in stream order.  A running
 *           maximum of off + n over the slots gives overlaps and gaps.
 *   order info (device int32 [8]): status, carriers, N, frame word 2, volume_id, first gap's first
 *           bit, first gap's end (exclusive), frame word 5.  Status: 0 ok, 1 no carrier, 2 carriers
 *           of different volumes (or a frame with B = 0 or N outside 1..2^31-1), 3 a duplicate index,
 *           an index or share out of range, or overlapping shares, 4 a gap.
 *   table   (device int32 [B][4]): per stack slice (index, off_b, n_b, 1 when it took its slot).
 *   gather  one thread per stream word: the slot by offset, then a walk; the share's rows start at
 *           word 3 of the user row.  Every word is written once, uncovered bits are zero; with a
 *           status other than 0 or 4 all words are zero.
 *
 * Workspace: codec_pee_blind_volume_workspace_bytes(P, tmax, max_entries) -- the blind auto
 * workspace, then the curve, the lengths, the skip marks, the user rows [B][P->payload_words] and
 * the slot tables.  It enters the PEE workspace registry as every workspace-taking entry does and
 * carries nothing from call to call behind that.  Decode-side calls pass tmax = 1.
 *
 * No kernel waits on another workgroup; none uses a fence or a global atomic; what crosses launches
 * goes through stream order.  Every value a kernel reads back from device memory is clamped to its
 * row, slice or table: lengths, frame words, indices, offsets, slots.
 *
 * Argument checks, in this order, before any device operation: params NULL, max_entries, tmax in
 * 1..16, codec_tcc_blind.h's list (H, W <= 65535, T <= 64, H W >= 192, the row width), then
 * B <= 65535 and B (H/2) (W/2) <= 2^31 - 1, P->payload_words >= 4 (extract side: user_words in
 * 3..2^24), nbits in 1..2^31 - 1, policy 0 or 1, stream_words in 0..2^25, NULL pointers, cover ==
 * stego, the workspace size.
 */
#ifndef CODEC_TCC_BLIND_VOL_H
#define CODEC_TCC_BLIND_VOL_H

#include "codec_tcc_blind_auto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_BVOL_PLAN 54   /* kernel tags of the profiling window (codec_profile_begin) */
#define CODEC_K_BVOL_ROWS 55
#define CODEC_K_BVOL_ORDER 56
#define CODEC_K_BVOL_GATHER 57

#define CODEC_PEE_BLIND_FLAG_VOLUME 4u /* header word 1, flag bit 2: the user bits start with a volume frame */
#define CODEC_PEE_BVOL_FRAME_WORDS 6
#define CODEC_PEE_BVOL_FRAME_BITS 192
#define CODEC_PEE_BVOL_FRAME_CRC 0x10000u /* frame word 2, bit 16 */
#define CODEC_PEE_BVOL_MAX_B 65535
#define CODEC_PEE_BVOL_INFO_WORDS 8
#define CODEC_PEE_BLIND_SKIPPED 3 /* per-slice info status: the volume plan gave the slice no bit */
#define CODEC_PEE_BVOL_OK 0
#define CODEC_PEE_BVOL_NO_CARRIER 1
#define CODEC_PEE_BVOL_MIXED 2
#define CODEC_PEE_BVOL_OVERLAP 3
#define CODEC_PEE_BVOL_GAP 4

size_t codec_pee_blind_volume_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries);

/* The plan alone, from a capacity curve [B][tmax] (codec_pee_blind_plan_auto's): n_out, off_out,
 * lengths_out (192 + n_b, 0 when skipped), skip_out: device int32 [B]; frames_out: device uint32 [B][6];
 * info: device int32 [8].  frame_crc: word 5 holds stream_crc (else 0). */
int codec_pee_blind_volume_plan(const codec_pee_params* P, const int32_t* curve, int32_t tmax, int64_t nbits,
                                int32_t policy, uint32_t volume_id, int32_t frame_crc, uint32_t stream_crc,
                                int32_t* n_out, int32_t* off_out, int32_t* lengths_out, int32_t* skip_out,
                                uint32_t* frames_out, int32_t* info, void* stream);

/* covers -> stegos, out of place.  bitstream: device uint64 [ceil(nbits / 64)], LSB first.  cover_crc
 * (or NULL): device uint32 [B], the covers' CRC-32 for header word 5 (sets flag bit 0).  slice_info:
 * device int32 [B][8] and t_out: device int32 [B] as codec_pee_blind_embed_auto's; meta, lm: its too. */
int codec_pee_blind_volume_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                                 int64_t nbits, int32_t policy, int32_t tmax, int32_t max_entries, uint32_t volume_id,
                                 int32_t frame_crc, uint32_t stream_crc, const uint32_t* cover_crc, int32_t* n_out,
                                 int32_t* off_out, uint32_t* frames_out, int32_t* info, int32_t* slice_info,
                                 int32_t* t_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* rows: device uint64 [B][user_words], the user rows codec_pee_blind_extract wrote (frame || share);
 * hdr: codec_pee_blind_headers' words; skip (or NULL): device int32 [B]. */
int codec_pee_blind_volume_order(const codec_pee_params* P, const uint64_t* rows, int32_t user_words,
                                 const uint32_t* hdr, const int32_t* skip, int32_t* info, int32_t* table_out,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* After an order on the same workspace: bitstream, device uint64 [stream_words]. */
int codec_pee_blind_volume_gather(const codec_pee_params* P, const uint64_t* rows, int32_t user_words,
                                  const int32_t* info, uint64_t* bitstream, int64_t stream_words, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Blind extract (skipped slices copied through), then order, then gather.  rows_out: device uint64
 * [B][user_words]. */
int codec_pee_blind_volume_extract(const codec_pee_params* P, const void* stego, const uint32_t* hdr,
                                   const codec_pee_meta* meta, const int32_t* skip, void* cover_out,
                                   uint64_t* rows_out, int32_t user_words, uint64_t* bitstream, int64_t stream_words,
                                   int32_t* info, int32_t* table_out, void* workspace, size_t workspace_bytes,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_BLIND_VOL_H */

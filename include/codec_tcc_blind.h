/*
 * codec_tcc_blind.h -- blind MED-PEE (scheme 1, fixed T): the stego alone carries its location
 * map and record.  Same boundary contract as codec_tcc.h and codec_tcc_roi.h (device pointers, a
 * caller-provided workspace, asynchronous on `stream`, no allocation, no host synchronisation,
 * capturable into a graph, 0 or a negative status with a codec_last_error text).
 *
 * The format (specification: tests/pee_blind_spec.py).  hc = H / 2, wc = W / 2.
 * A slice carries n_side = 192 + 32 E side bits; side bit i is bit 0 of the pixel with flat
 * index H W - 1 - i, 32-bit words LSB first:
 *   word 0 magic 0x4D504231; 1 T | flags << 8 | maxval << 16 (flag bit 0: word 5 holds the
 *   cover's CRC-32); 2 n_user; 3 E; 4 end (0xFFFFFFFF for -1); 5 the CRC or 0; 6 .. 5 + E the
 *   ascending candidate indices of the location map's set bits up to `end`, then 0xFFFFFFFF.
 * The plan, per slice and from the cover alone: cap_i / uns_i = cumulative counts through candidate
 * row i of expandable-and-safe / unsafe candidates at P->T; i* = the first row with
 * cap_i >= n_user + 192 + 32 uns_i; E = uns_{i*}; r = ceil(n_side / (2 W)); the rows from
 * 2 (hc - r) on are reserved: the ROI embed (codec_pee_roi_embed) neither modifies them nor uses
 * them as context of a candidate it touches, so their LSBs hold the side bits and the LSBs they
 * displace lead the PEE payload.  Status 1 (capacity): no row qualifies or i* >= hc - r; status 2:
 * E > max_entries.  A refused slice is copied through and carries no header.
 *
 * info: device int32 [B][8] = (status, n_user, E, n_side, end, region row 2 (hc - r), i*,
 * the largest n_user that would fit or -1).  A refused slice has n_side 0, end -1, row 0.
 *
 * Workspace: codec_pee_blind_workspace_bytes(P, max_entries) with P->payload_words = the PEE
 * payload row, CODEC_PEE_BLIND_ROW_WORDS(max n_user, max_entries) words or more.  It starts with
 * a codec_pee workspace of P (the ROI calls run on it; it enters the PEE workspace registry as
 * every workspace-taking entry does) and carries nothing from call to call behind it.
 *
 * No kernel of this unit waits on another workgroup; what crosses launches goes through stream
 * order.  Whatever the device-resident values hold (lengths, header words, entries), the kernels
 * address nothing outside the slices, the rows and the map: they clamp.
 *
 * Argument checks, in this order, before any device operation: params NULL, max_entries, the
 * params' own ranges (codec_tcc.h), H, W <= 65535, T <= 64, H W >= 192, the row width, NULL
 * pointers, the call's own rules, the workspace size.
 */
#ifndef CODEC_TCC_BLIND_H
#define CODEC_TCC_BLIND_H

#include "codec_tcc_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_BLIND_ROWS 52 /* read-only pass: per-candidate-row counts (expandable and safe, unsafe) */

#define CODEC_PEE_BLIND_MAGIC 0x4D504231u
#define CODEC_PEE_BLIND_HDR_WORDS 6
#define CODEC_PEE_BLIND_MAX_ENTRIES 65536
#define CODEC_PEE_BLIND_INFO_WORDS 8
#define CODEC_PEE_BLIND_FLAG_CRC 1
/* uint64 words of the PEE payload row that holds the side bits and n_user user bits */
#define CODEC_PEE_BLIND_ROW_WORDS(n_user, max_entries) (((long long)(n_user) + 192 + 32LL * (max_entries) + 63) / 64)

size_t codec_pee_blind_workspace_bytes(const codec_pee_params* P, int32_t max_entries);

/* Row table + plan alone: info[b] for lengths[b] user bits (lengths NULL: 0 bits each), whose last
 * word is the slice's capacity.  Read-only on the cover. */
int codec_pee_blind_plan(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t max_entries,
                         int32_t* info, void* workspace, size_t workspace_bytes, void* stream);

/* cover -> stego, out of place (cover != stego): row table, plan, splice (displaced LSBs || user
 * bits into the workspace's rows), codec_pee_roi_embed on those rows, pack (header, entries and
 * padding into the stego's LSBs; info's `end`).  payload: device [B][user_words] uint64, lengths:
 * device int32 [B] user bits (clamped to 0 .. 64 user_words); crc: device uint32 [B] cover CRC-32
 * (codec_crc32_slices) or NULL (flag bit 0 clear, word 5 = 0).  meta / lm: the ROI embed's
 * records and maps ([B] / [B][lm_words]), kept for callers that want them beside the stego. */
int codec_pee_blind_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                          int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t max_entries,
                          int32_t* info, codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes,
                          void* stream);

/* hdr_out: device uint32 [B][8] = side words 0 .. 5 of every slice, then two zeros.  No workspace. */
int codec_pee_blind_headers(const codec_pee_params* P, const void* stego, uint32_t* hdr_out, void* stream);

/* stego -> cover_out + user bits.  hdr: what codec_pee_blind_headers wrote (device); meta: device
 * [B] records rebuilt from the checked headers (the host layer builds them: T, maxval, L = n_side
 * + n_user, end, the reserved rectangle in reserved[0] / [2], reserved[1] = 65536).  The call
 * zeroes the workspace's map and scatters the entries into it, runs codec_pee_roi_extract into
 * the workspace's rows (P->payload_words wide), writes the first n_side extracted bits back into
 * cover_out's LSBs and the rest, shifted down, into payload_out [B][user_words] (whole rows are
 * written; bits past n_user are 0). */
int codec_pee_blind_extract(const codec_pee_params* P, const void* stego, const uint32_t* hdr,
                            const codec_pee_meta* meta, void* cover_out, uint64_t* payload_out, int32_t user_words,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_BLIND_H */

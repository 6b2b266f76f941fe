/*
 * codec_tcc_blind_auto.h -- blind MED-PEE with capacity control: T chosen per slice on the device.
 * The entries stand beside those of codec_tcc_blind.h and share its boundary contract (device
 * pointers, a caller-provided workspace, asynchronous on `stream`, no allocation, no host
 * synchronisation, capturable into a graph, 0 or a negative status with a codec_last_error text).
 * The format is codec_tcc_blind.h's: what these entries write, codec_pee_blind_headers and
 * codec_pee_blind_extract read, T from each slice's header.
 *
 * The rule (specification: tests/pee_blind_auto_spec.py), per slice: T* is the
 * smallest T in 1..tmax whose plan (codec_tcc_blind.h) for the slice's n_user has status 0; the
 * slice is embedded exactly as codec_pee_blind_embed at P->T = T* embeds it.  Nothing is assumed
 * monotone in T: a shift by T can leave the range, so the unsafe counts, E, r and the status
 * change from one T to the next.  When no T qualifies the slice is refused: copied through, no
 * header, the info of the plan at T = tmax, t_out 0.
 *
 * One read-only pass over the cover (kernel tag CODEC_K_BLIND_ROWS_AUTO) classifies each candidate
 * once and writes its row's counts at every T: the table [B][tmax][hc] of (expandable and safe,
 * unsafe) pairs.  One workgroup per slice then applies the plan at T = 1 .. tmax in turn.
 *
 * info: device int32 [B][8] as codec_tcc_blind.h's, of the plan at T* (at tmax when refused),
 * except the last word: the largest capacity over T = 1..tmax, -1 when no T takes even 0 bits.
 * t_out: device int32 [B], T* or 0.  curve: device int32 [B][tmax], the capacity at each T, or NULL.
 *
 * Workspace: codec_pee_blind_auto_workspace_bytes(P, tmax, max_entries): the blind workspace with
 * a row table tmax times as large.  It starts with a codec_pee workspace of P and enters the PEE
 * workspace registry as every workspace-taking entry does; it carries nothing from call to call
 * behind that.  P->T is only range-checked.
 *
 * No kernel waits on another workgroup and none uses a global atomic or a fence; what crosses
 * launches goes through stream order.  Lengths, table entries and the chosen T are clamped to the
 * row, the candidates of a row and 1..64 wherever a kernel reads them back from device memory.
 *
 * Argument checks, in this order, before any device operation: params NULL, max_entries, tmax in
 * 1..16, then codec_tcc_blind.h's list from the params' own ranges on (H, W <= 65535, T <= 64,
 * H W >= 192, the row width, NULL pointers, the call's own rules, the workspace size).
 */
#ifndef CODEC_TCC_BLIND_AUTO_H
#define CODEC_TCC_BLIND_AUTO_H

#include "codec_tcc_blind.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_BLIND_ROWS_AUTO 53 /* read-only pass: per-candidate-row counts at every T in 1..tmax */

#define CODEC_PEE_BLIND_TMAX 16

size_t codec_pee_blind_auto_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries);

/* Row table + plan alone (lengths NULL: 0 bits each).  Read-only on the cover. */
int codec_pee_blind_plan_auto(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t tmax,
                              int32_t max_entries, int32_t* info, int32_t* t_out, int32_t* curve, void* workspace,
                              size_t workspace_bytes, void* stream);

/* cover -> stego, out of place: codec_pee_blind_embed with T chosen per slice.  The arguments are
 * codec_pee_blind_embed's, with tmax and t_out added. */
int codec_pee_blind_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                               int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t tmax,
                               int32_t max_entries, int32_t* info, int32_t* t_out, codec_pee_meta* meta, uint64_t* lm,
                               void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_BLIND_AUTO_H */

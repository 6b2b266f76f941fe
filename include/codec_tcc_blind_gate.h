/*
 * codec_tcc_blind_gate.h -- gated blind MED-PEE: (T, gate) chosen per slice on the device, the gate
 * carried in the slice's header.  The entries stand beside those of codec_tcc_blind_auto.h and share
 * their boundary contract (device pointers, a caller-provided workspace, asynchronous on `stream`, no
 * allocation, no host synchronisation, capturable into a graph, 0 or a negative status with a
 * codec_last_error text).
 *
 * The scheme (specification: tests/pee_blind_gate_spec.py).  The gate is a value of
 * codec_tcc_gate.h's ladder, G = GATES[j], j in 0..15; a candidate is active iff its roughness
 * D = max(W, N, NW) - min(W, N, NW) <= G.  The plan at (T, j) is codec_tcc_blind.h's with gated counts:
 * cap_i counts the candidates through row i that are active, expandable and safe, uns_i those that are
 * active and unsafe; i*, E, n_side, r, the rectangle, the statuses and the capacity follow as there.
 * The rule, per slice, over T in 1..tmax and j in 0..15: the smallest T for which some j has a plan of
 * status 0, and at that T the smallest such j; nothing is assumed monotone in T or j.  t_fixed > 0 fixes
 * T (1..tmax), j_fixed >= 0 fixes j; 0 and -1 mean "free".  When no pair qualifies the slice is refused:
 * copied through, no header, the info of the plan at the last pair considered (tmax, j = 15, or the
 * fixed values), t_out 0, g_out -1.
 *
 * The format is codec_tcc_blind.h's with two flag fields more: flag bit 3 (CODEC_PEE_BLIND_FLAG_GATED)
 * marks a gated slice, and flag bits 4-7 then hold j (also at j = 15).  Without bit 3, bits 4-7 are 0.
 * codec_pee_blind_headers and codec_pee_blind_extract read such a slice as they read any other: the
 * record the host layer rebuilds carries reserved[1] = GATES[j] + 1, and the ROI extract does the rest.
 *
 * One read-only pass over the cover (kernel tag CODEC_K_BLIND_ROWS_GATE) classifies each candidate
 * once and writes, per candidate row, its counts at every (T, class <= j): the table
 * [B][tmax][16][hc] of 32-bit words cap | uns << 16 (a row has at most 32767 candidates).  At
 * tmax = 16 and 256 slices of 2048 x 2048 that table is 256 MB; at the Python layer's default
 * tmax = 4 it is 64 MB.  One workgroup per slice then applies the plan to every pair and the rule.
 *
 * info: device int32 [B][8] as codec_tcc_blind.h's, of the plan at the chosen pair (the last pair
 * considered when refused), except the last word: the largest capacity over the pairs considered, -1 when
 * none takes even 0 bits.  t_out: device int32 [B], T* or 0.  g_out: device int32 [B], GATES[j*] or -1.
 * curve: device int32 [B][tmax][16], the capacity at every pair (whatever is fixed), or NULL.
 *
 * Workspace: codec_pee_blind_gate_workspace_bytes(P, tmax, max_entries): the blind workspace with that
 * table and one flag word per slice.  It starts with a codec_pee workspace of P and enters the PEE
 * workspace registry as every workspace-taking entry does; it carries nothing from call to call behind
 * that.  P->T is only range-checked.
 *
 * No kernel waits on another workgroup and none uses a global atomic or a fence; what crosses launches
 * goes through stream order.  Lengths, table entries and the chosen pair are clamped to the row, the
 * candidates of a row, 1..64 and the ladder wherever a kernel reads them back from device memory.
 *
 * Argument checks, in this order, before any device operation: params NULL, max_entries, tmax in
 * 1..16, then codec_tcc_blind.h's list from the params' own ranges on (H, W <= 65535, T <= 64,
 * H W >= 192, the row width), t_fixed in 0..tmax, j_fixed in -1..15, NULL pointers, the call's own
 * rules, the workspace size.
 */
#ifndef CODEC_TCC_BLIND_GATE_H
#define CODEC_TCC_BLIND_GATE_H

#include "codec_tcc_blind_auto.h"
#include "codec_tcc_gate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_BLIND_ROWS_GATE 58 /* read-only pass: per-candidate-row counts at every (T, gate class) */

#define CODEC_PEE_BLIND_FLAG_GATED 8
#define CODEC_PEE_BLIND_FLAG_GATE_SHIFT 4

size_t codec_pee_blind_gate_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries);

/* Table + plan alone (lengths NULL: 0 bits each).  Read-only on the cover. */
int codec_pee_blind_plan_gate(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t tmax,
                              int32_t t_fixed, int32_t j_fixed, int32_t max_entries, int32_t* info, int32_t* t_out,
                              int32_t* g_out, int32_t* curve, void* workspace, size_t workspace_bytes, void* stream);

/* cover -> stego, out of place: codec_pee_blind_embed_auto with the pair chosen per slice.  The arguments
 * are codec_pee_blind_embed_auto's, with t_fixed, j_fixed and g_out added. */
int codec_pee_blind_embed_gate(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                               int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t tmax,
                               int32_t t_fixed, int32_t j_fixed, int32_t max_entries, int32_t* info, int32_t* t_out,
                               int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_BLIND_GATE_H */

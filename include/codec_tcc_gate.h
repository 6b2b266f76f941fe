/*
 * codec_tcc_gate.h -- smoothness-gated MED-PEE (scheme 1): embed only where the MED context is
 * flat.  Same boundary contract as codec_tcc.h (device pointers, a caller-provided workspace,
 * asynchronous on `stream`, no allocation, no host synchronisation, capturable into a graph,
 * 0 or a negative status with a codec_last_error text).
 *
 * The scheme (all integer; specification: tests/pee_gate_spec.py, scalar restatement in the
 * same file).  A candidate's roughness is D = max(a, b, c) - min(a, b, c) of its W, N and NW
 * neighbours -- pixels scheme 1 never modifies, so the decoder sees the same D.  With a gate G
 * in 0..65535 a candidate is ACTIVE iff D <= G.  Inactive candidates are never modified, their
 * location-map bit is 0, they carry no bit and count towards nothing (capacity, the bit cursor,
 * lm_count, the decoder's inner-candidate counts).  Active candidates follow codec_pee_embed
 * exactly (classification, expansion / shifting, the overflow map, the bit order, `end` = the
 * index of the candidate carrying bit L - 1, truncation with end = nc - 1 and status 1).
 * G = 65535 is codec_pee_embed bit for bit.  The record carries the gate:
 * codec_pee_meta.reserved[1] = G + 1; 0 = ungated, which is every record written before.
 *
 * Capacity table.  GATES = 0 1 2 3 4 6 8 12 16 24 32 48 64 96 128 65535; a candidate's class is
 * the first j with D <= GATES[j].  Per slice
 *   n[j]     = candidates of class j,
 *   hs[u][j] = those of class j whose expansion stays in [0, maxval] (codec_pee_capacity's
 *              test) and whose folded error u = (e >= 0 ? e : -e - 1) is below tmax,
 *   K(T, j)  = sum of hs[u][g] over u < T, g <= j = the capacity at (T, GATES[j]),
 *   N(j)     = sum of n[g] over g <= j.
 * Selection (tmax <= 16 and (H/2)(W/2) <= 2^26, so that every product fits 64 unsigned bits):
 *   A(T, j)  = 2 T^2 (N(j) - K(T, j)) + sum over u < T, g <= j of hs[u][g] (u^2 + (u+1)^2),
 *              twice the expected squared error of processing the whole slice;
 *   among the pairs with K >= L and K > 0 the smallest A / K (A1 K2 < A2 K1, exactly), ties to
 *   the smaller T, then the smaller j; L = 0 gives (1, 0); no feasible pair gives T = tmax,
 *   j = 15: the ungated truncated embedding.
 *   t_fixed > 0 restricts the rule to that T.  g_fixed >= 0 replaces the ladder by the two
 *   classes D <= g_fixed (column 0) and the rest (column 15) and picks the smallest T whose
 *   K(T, 0) holds L (tmax if none), with the gate g_fixed.
 */
#ifndef CODEC_TCC_GATE_H
#define CODEC_TCC_GATE_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_PEE_GATE_TABLE 41 /* read-only pass: gated capacity table + selection tail */

#define CODEC_PEE_GATE_CLASSES 16
#define CODEC_PEE_GATE_TMAX 16
#define CODEC_PEE_GATE_MAX 65535
#define CODEC_PEE_GATE_MAX_NC (1 << 26)

/* Bytes of the workspace of the gated calls: codec_pee_workspace_bytes(P) followed by the
 * table's bins.  Every codec_pee_* call accepts it (it is a codec_pee workspace with a tail),
 * and the rules of codec_pee_workspace_bytes hold for it unchanged: zero it once
 * (codec_pee_reset), keep one per stream.  The tail carries no state between calls.  0 for
 * bad arguments (tmax outside 1..16 included). */
size_t codec_pee_gate_workspace_bytes(const codec_pee_params* P, int32_t tmax);

/* One read-only pass over the covers.  n [B][16] and hs [B][tmax][16] (device uint32; either
 * may be NULL) receive the table.  lengths (device int32 [B], bits per slice; may be NULL)
 * switches the selection on: t_out[B], g_out[B] (the chosen T and gate VALUE, GATES[j]) and
 * k_out[B] (the capacity K at the choice), each device int32 and each optional.  t_fixed: 0, or
 * the only T considered (1..tmax).  g_fixed: -1 for the ladder, or a gate 0..65535 (see above).
 * P->T is not used (but checked, as by every entry: >= 1).  The call enters the workspace's
 * shape record like every codec_pee call (codec_pee_workspace_bytes, "shape change"): its bins lie
 * behind P's layout, which on a workspace in use for a larger shape is inside that shape's
 * state, so the larger shape's next call zeroes the workspace first. */
int codec_pee_gate_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed,
                            int32_t g_fixed, const int32_t* lengths, uint32_t* n, uint32_t* hs, int32_t* t_out,
                            int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes, void* stream);

/* codec_pee_embed_ts with a gate per slice: t_slices[B] (>= 1) and g_slices[B] (0..65535),
 * device int32, both required.  stego == cover is allowed.  Writes meta.reserved[1] = G + 1.
 * workspace: codec_pee_workspace_bytes(P) bytes or more. */
int codec_pee_gate_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                         const int32_t* lengths, const int32_t* t_slices, const int32_t* g_slices,
                         codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes, void* stream);

/* codec_pee_gate_capacity (with lengths) -> codec_pee_gate_embed on one stream, results
 * identical to the two calls.  t_out and g_out are required (the embed reads them).
 * workspace: codec_pee_gate_workspace_bytes(P, tmax). */
int codec_pee_gate_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                              const int32_t* lengths, int32_t tmax, int32_t t_fixed, int32_t g_fixed, int32_t* t_out,
                              int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                              size_t workspace_bytes, void* stream);

/* codec_pee_extract with T and the gate taken from each record (reserved[1] = G + 1; a record
 * with reserved[1] = 0 decodes ungated).  The record contract of codec_pee_extract holds.
 * workspace: codec_pee_workspace_bytes(P) bytes or more. */
int codec_pee_gate_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta,
                           const uint64_t* lm, void* cover_out, uint64_t* payload_out, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_GATE_H */

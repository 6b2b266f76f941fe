/*
 * codec_tcc_roi.h -- ROI-protected MED-PEE (scheme 1): a per-slice rectangle that the embed
 * never modifies, and the kernel that finds one.  Same boundary contract as codec_tcc.h and
 * codec_tcc_gate.h (device pointers, a caller-provided workspace, asynchronous on `stream`, no
 * allocation, no host synchronisation, capturable into a graph, 0 or a negative status with a
 * codec_last_error text).
 *
 * The scheme (specification: tests/pee_roi_spec.py).  The ROI of slice b is a half-open pixel
 * rectangle (y0, x0, y1, x1), 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W; one with y0 == y1 or
 * x0 == x1 is empty and counts as (0, 0, 0, 0).  Candidate (i, j) sits at pixel (2i+1, 2j+1)
 * and is PROTECTED iff y0 <= 2i+1 < y1 and x0 <= 2j+1 < x1.  A candidate is ACTIVE iff it is not
 * protected and its roughness D <= G (codec_tcc_gate.h; G = 65535 when no gate is wanted).
 * Inactive candidates behave as in codec_tcc_gate.h: never modified, location-map bit 0, they
 * carry no bit and count towards nothing; `end` still indexes all candidates.  Scheme 1 never
 * modifies a non-candidate, so the stego equals the cover on every pixel of the rectangle.
 * Protected pixels still serve as MED context outside it: neither side modifies them.
 *
 * The record carries the rectangle as unsigned bit patterns:
 *   codec_pee_meta.reserved[0] = (y0 << 16) | x0,  reserved[2] = (y1 << 16) | x1,
 *   reserved[1] = G + 1 (always written: 65536 when no gate was asked for).
 * reserved[2] == 0 means "no ROI": every record written before has it.  Hence H, W <= 65535.
 *
 * Capacity table and selection: protected candidates fall into no class (absent from n[] and
 * hs[][]); the rule of codec_tcc_gate.h then applies unchanged.
 *
 * The rectangle array `roi` is DEVICE memory, int32 [B][4] as (y0, x0, y1, x1), NULL for none.
 * The library cannot check its values on the host (the host layer does: codec_tcc_amd/roi.py);
 * whatever it holds, the kernels address nothing outside the slice: a rectangle only changes
 * which candidates count as active.  A row with a negative value, y0 >= y1, x0 >= x1 or a value
 * above 65535 counts as no rectangle, and the record says so (reserved[2] = 0).  Both sides derive
 * the protected candidates from the two record words, so an embed and the extract of its records
 * always agree.
 *
 * Argument checks, in this order, before any device operation: params (NULL, tmax, t_fixed,
 * g_fixed, the candidate limit: codec_tcc_gate.h's), the params' own ranges (codec_tcc.h),
 * H, W <= 65535, NULL pointers, the call's own rules, the workspace size.
 */
#ifndef CODEC_TCC_ROI_H
#define CODEC_TCC_ROI_H

#include "codec_tcc_gate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_ROI_BBOX 46 /* read-only pass: per-slice bounding rectangle of the pixels > level */

#define CODEC_PEE_ROI_MAX_DIM 65535

/* codec_pee_gate_capacity with the slices' rectangles.  workspace: codec_pee_gate_workspace_bytes. */
int codec_pee_roi_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed,
                           int32_t g_fixed, const int32_t* lengths, const int32_t* roi, uint32_t* n, uint32_t* hs,
                           int32_t* t_out, int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* codec_pee_gate_embed with the slices' rectangles.  Writes all three reserved words (above).
 * The routes are the gated call's (two-pass kernels and the look-back single pass; the call
 * zeroes its status words first).  workspace: codec_pee_workspace_bytes(P) bytes or more. */
int codec_pee_roi_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                        const int32_t* lengths, const int32_t* t_slices, const int32_t* g_slices, const int32_t* roi,
                        codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes, void* stream);

/* codec_pee_roi_capacity (with lengths) -> codec_pee_roi_embed on one stream.
 * workspace: codec_pee_gate_workspace_bytes(P, tmax). */
int codec_pee_roi_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                             const int32_t* lengths, int32_t tmax, int32_t t_fixed, int32_t g_fixed, const int32_t* roi,
                             int32_t* t_out, int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                             size_t workspace_bytes, void* stream);

/* codec_pee_gate_extract that also takes the rectangle from each record.  It reads every earlier
 * scheme-1 record (those have reserved[2] == 0).  codec_pee_gate_extract itself keeps ignoring
 * reserved[0] and reserved[2]. */
int codec_pee_roi_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta,
                          const uint64_t* lm, void* cover_out, uint64_t* payload_out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Per slice, the tight bounding rectangle of the pixels with value > level, grown by
 * margin >= 0 pixels on every side and clamped to the image, as (y0, x0, y1, x1) half-open; a
 * slice without such a pixel gives (0, 0, 0, 0).  image: device [B][H][W] of P->bytes (1 or 2)
 * bytes per pixel; roi_out: device int32 [B][4].  One read-only pass (16-byte loads when the
 * image is 16-byte aligned and a row is a whole number of them, scalar loads otherwise) between
 * a launch that initialises roi_out as the accumulator and one that finishes it: no memset, no
 * workspace.  Only B, H, W and bytes of P are used (all of P is checked; H, W <= 65535);
 * level in 0..65535, margin in 0..65535. */
int codec_roi_bbox(const codec_pee_params* P, const void* image, int32_t level, int32_t margin, int32_t* roi_out,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_ROI_H */

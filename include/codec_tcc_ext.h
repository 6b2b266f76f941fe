/*
 * codec_tcc_ext.h -- entries of libcodec_hip.so added after codec_tcc.h's list was fixed.
 * Same boundary contract as codec_tcc.h (device pointers, asynchronous on `stream`, 0 or a
 * negative status with a codec_last_error text).
 */
#ifndef CODEC_TCC_EXT_H
#define CODEC_TCC_EXT_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Capacity-controlled scheme 2: t_out[B] (device int32, required) receives per slice the
 * smallest T in [tmin, tmax] (1 <= tmin <= tmax <= 64) whose four passes hold lengths[b] bits,
 * tmax if none does (the slice is then truncated exactly as codec_pee_multi_embed at tmax);
 * stego / metas [4][B] / lm [4][B][lm_words] equal codec_pee_multi_embed run on that slice
 * with P->T = t_out[b] (P->T itself is ignored; meta.T records the choice, the extract reads it
 * there).  Out of place only (a failed trial is undone from the cover): cover == stego is an
 * argument error.  One launch, one workgroup per slice, for every batch shape: built for
 * chip-filling batches of small slices; a few large slices run on as many CUs.  Capture-safe;
 * keeps no state in the workspace.  Specification: the T scan over oracle/pee_cpu.py
 * pee_embed_multi (no reference counterpart). */
#define CODEC_K_PEE_LAT_AUTO 35
int codec_pee_multi_embed_auto(const codec_pee_params* P, const void* cover, void* stego,
                               const uint64_t* payload, const int32_t* lengths, int32_t tmin,
                               int32_t tmax, int32_t* t_out, codec_pee_meta* metas, uint64_t* lm,
                               void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_EXT_H */

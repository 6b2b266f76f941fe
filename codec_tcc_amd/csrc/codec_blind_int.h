// codec_blind_int.h -- what codec_blind.hip offers the other translation units of the library
// (codec_bvol.hip): the blind workspace layout, the entries' shared checks and the launch sequences
// behind codec_pee_blind_embed_auto and codec_pee_blind_extract, cut where a volume plan goes between
// them.  The kernels stay in codec_blind.hip; these are host functions.
#pragma once
#include "codec_common.h"
#include "codec_tcc_blind.h"
#include "codec_tcc_blind_auto.h"

struct BlWs {
    size_t rows, rect, lens, ts, gs, lm, pay, total;
};
// the layout behind the codec_pee workspace of P (base = codec_pee_workspace_bytes(P) > 0); the row
// table holds `tables` T's
static inline BlWs bl_ws(const codec_pee_params* P, size_t base, int tables = 1) {
    BlWs L;
    const size_t B = (size_t)P->B;
    size_t o = align_up(base, 256);
    L.rows = o; o += align_up(B * (size_t)tables * (size_t)(P->H / 2 > 0 ? P->H / 2 : 1) * 8, 256);
    L.rect = o; o += align_up(B * 16, 256);
    L.lens = o; o += align_up(B * 4, 256);
    L.ts = o; o += align_up(B * 4, 256);
    L.gs = o; o += align_up(B * 4, 256);
    L.lm = o; o += align_up(B * (size_t)P->lm_words * 8, 256);
    L.pay = o; o += align_up(B * (size_t)P->payload_words * 8, 256);
    L.total = o;
    return L;
}

// the checks every blind entry shares; `ws`: the entry takes the workspace
int blind_check(const codec_pee_params* P, int32_t max_entries, bool ws, size_t* base, const char* who, int32_t tmax = 1);

// the table [B][tmax][hc] of the row counts at every T in 1..tmax: the one pass over the cover
int blind_rows_auto(const codec_pee_params* P, const BlWs& L, const void* cover, int32_t tmax, char* ws, hipStream_t st);

// the per-slice plan over that table (k_blind_plan_auto).  skip (or NULL): device int32 [B]; a slice
// with a nonzero entry is refused with status CODEC_PEE_BLIND_SKIPPED whatever its capacity
int blind_plan_table(const codec_pee_params* P, const BlWs& L, const int32_t* lengths, const int32_t* skip, int user_bits,
                     int frame_bits, long long row_bits, int32_t tmax, int32_t max_entries, int32_t* info, int32_t* t_out,
                     int32_t* curve, char* ws, hipStream_t st);

// after a plan: splice, the ROI embed on the plan's arrays, pack
int blind_embed_planned(const codec_pee_params* P, const BlWs& L, const void* cover, void* stego, const uint64_t* payload,
                        int32_t user_words, const uint32_t* frames, const uint32_t* crc, uint32_t flags, int32_t* info,
                        codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes, void* stream);

// codec_pee_blind_extract's launches after its checks and pee_workspace_enter.  skip (or NULL): device
// int32 [B]; a slice with a nonzero entry carries no header: no entry is scattered, no LSB restored,
// its user row is zero (its record must copy the slice through)
int blind_extract_launch(const codec_pee_params* P, const BlWs& L, const void* stego, const uint32_t* hdr,
                         const codec_pee_meta* meta, const int32_t* skip, void* cover_out, uint64_t* payload_out,
                         int32_t user_words, void* workspace, size_t workspace_bytes, void* stream);

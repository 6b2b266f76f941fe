// codec_blind_int.h -- what codec_blind.hip offers the other translation units of the library
// (codec_bvol.hip, codec_blind_gate.hip): the blind workspace layout, the entries' shared checks and the
// launch sequences behind codec_pee_blind_embed_auto and codec_pee_blind_extract, cut where a volume plan
// goes between them; and the device functions of the plan rule, which codec_blind_gate.hip's plan kernel
// runs over its own table.  The kernels stay in codec_blind.hip.
#pragma once
#include <limits.h>

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

// after a plan: splice, the ROI embed on the plan's arrays, pack.  flags_b (or NULL): device uint32 [B],
// flag bits of each slice's own, or-ed into the header's beside `flags`
int blind_embed_planned(const codec_pee_params* P, const BlWs& L, const void* cover, void* stego, const uint64_t* payload,
                        int32_t user_words, const uint32_t* frames, const uint32_t* crc, uint32_t flags, int32_t* info,
                        codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes, void* stream,
                        const uint32_t* flags_b = nullptr);

// codec_pee_blind_extract's launches after its checks and pee_workspace_enter.  skip (or NULL): device
// int32 [B]; a slice with a nonzero entry carries no header: no entry is scattered, no LSB restored,
// its user row is zero (its record must copy the slice through)
int blind_extract_launch(const codec_pee_params* P, const BlWs& L, const void* stego, const uint32_t* hdr,
                         const codec_pee_meta* meta, const int32_t* skip, void* cover_out, uint64_t* payload_out,
                         int32_t user_words, void* workspace, size_t workspace_bytes, void* stream);

// ---- device functions (every includer is a HIP unit)
#define BL_HDR_BITS 192

__device__ __forceinline__ int bl_med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), a + b - c)); }

template <typename V> __device__ __forceinline__ uint32_t bl_px(const V& v, int e);
template <> __device__ __forceinline__ uint32_t bl_px<uint4>(const uint4& v, int e) {
    const uint32_t w = e < 2 ? v.x : (e < 4 ? v.y : (e < 6 ? v.z : v.w));
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
template <> __device__ __forceinline__ uint32_t bl_px<uint2>(const uint2& v, int e) {
    return ((e < 4 ? v.x : v.y) >> (8 * (e & 3))) & 0xFFu;
}

// the plan of one slice at one T
struct BlPlan {
    int status, E, n_side, istar, y0, cap;
};

// one row of the plan rule: the row's counts through row i -> (side bits, room for user bits, rows reserved)
struct BlRow {
    long long side, room, rr;
};
__device__ __forceinline__ BlRow bl_plan_row(uint32_t cap, uint32_t uns, int W) {
    BlRow r;
    r.side = BL_HDR_BITS + 32LL * uns;
    r.room = (long long)cap - r.side;
    r.rr = (r.side + 2LL * W - 1) / (2LL * W);
    return r;
}
// the largest n_user the row would take, or -1
__device__ __forceinline__ int bl_plan_cap(const BlRow& r, int i, uint32_t uns, int hc, int max_entries, long long row_bits) {
    return (i < hc - r.rr && uns <= (uint32_t)max_entries && r.side <= row_bits && r.room >= 0)
               ? (int)min(r.room, row_bits - r.side) : -1;
}
// the plan from the first row that has room (first = row << 32 | unsafe through it, or ~0) and the capacity
__device__ __forceinline__ BlPlan bl_plan_decide(u64 first, int cap, int hc, long long n_user, int W, int max_entries, long long row_bits) {
    BlPlan p = {0, 0, 0, -1, 0, cap};
    if (first == ~0ull) {
        p.status = 1;
    } else {
        p.istar = (int)(first >> 32);
        const long long e = (long long)(first & 0xFFFFFFFFull);
        const long long side = BL_HDR_BITS + 32 * e;
        const long long rr = (side + 2LL * W - 1) / (2LL * W);
        p.E = (int)min(e, (long long)INT_MAX);
        if (p.istar >= hc - rr) p.status = 1;
        else if (e > max_entries) p.status = 2;
        else if (side + n_user > row_bits) p.status = 1;   // a row narrower than the call's lengths: the host sizes it
        else { p.n_side = (int)side; p.y0 = 2 * (hc - (int)rr); }
    }
    return p;
}

// the plan rule over one slice's row counts at one T (row_at(i): row i's (expandable and safe, unsafe)) by
// one wave, with shuffles alone: no shared memory, no barrier.  An entry is clamped to the row's W / 2 candidates.
template <class Load>
__device__ __forceinline__ BlPlan bl_plan_rows_wave_by(Load row_at, int hc, long long n_user, int W, int max_entries,
                                                       long long row_bits) {
    const int lane = threadIdx.x & 63;
    const uint32_t wc = (uint32_t)W / 2;
    uint32_t cap0 = 0, uns0 = 0;
    int best = -1;
    u64 first = ~0ull;
    for (int c0 = 0; c0 < hc; c0 += 64) {
        const int i = c0 + lane;
        uint2 v = i < hc ? row_at(i) : make_uint2(0u, 0u);
        v.x = min(v.x, wc);
        v.y = min(v.y, wc);
        const uint32_t cap = cap0 + wave_incl_scan(v.x), uns = uns0 + wave_incl_scan(v.y);   // through row i
        bool hit = false;
        if (i < hc) {
            const BlRow r = bl_plan_row(cap, uns, W);
            best = max(best, bl_plan_cap(r, i, uns, hc, max_entries, row_bits));
            hit = r.room >= n_user;
        }
        const u64 hits = __ballot(hit);
        if (first == ~0ull && hits) {   // uniform: the first row with room, and the unsafe count through it
            const int l = __ffsll((long long)hits) - 1;
            first = ((u64)(uint32_t)(c0 + l) << 32) | (uint32_t)__shfl(uns, l, 64);
        }
        cap0 = (uint32_t)__shfl(cap, 63, 64);
        uns0 = (uint32_t)__shfl(uns, 63, 64);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    return bl_plan_decide(first, best, hc, n_user, W, max_entries, row_bits);
}

// info and the ROI embed's arrays of slice b (one thread); thr, gate: the T and the gate the ROI embed takes
__device__ __forceinline__ void bl_plan_write(int b, const BlPlan& p, long long n_user, int thr, int cap, int H, int W,
                              int32_t* __restrict__ info, int32_t* __restrict__ rect, int32_t* __restrict__ lens,
                              int32_t* __restrict__ ts, int32_t* __restrict__ gs, int gate = CODEC_PEE_GATE_MAX) {
    int32_t* I = info + (size_t)b * CODEC_PEE_BLIND_INFO_WORDS;
    I[0] = p.status; I[1] = (int)n_user; I[2] = p.E; I[3] = p.n_side; I[4] = -1; I[5] = p.y0; I[6] = p.istar; I[7] = cap;
    const bool ok = p.status == 0;
    rect[4 * b] = ok ? p.y0 : 0; rect[4 * b + 1] = 0; rect[4 * b + 2] = ok ? H : 0; rect[4 * b + 3] = ok ? W : 0;
    lens[b] = ok ? p.n_side + (int)n_user : 0;
    ts[b] = thr;
    gs[b] = gate;
}

// n_user of slice b: lengths NULL: 0 user bits; else the length clamped to 0 .. user_bits, behind
// frame_bits bits of frame (0, or a keyed slice's 224)
__device__ __forceinline__ long long bl_n_user(const int32_t* __restrict__ lengths, int b, int user_bits, int frame_bits) {
    return lengths ? (long long)frame_bits + (long long)min(max(lengths[b], 0), user_bits) : 0;
}

static __device__ __forceinline__ BlPlan bl_plan_rows_wave(const uint2* __restrict__ rows, int hc, long long n_user, int W,
                                                            int max_entries, long long row_bits) {
    return bl_plan_rows_wave_by([&](int i) { return rows[i]; }, hc, n_user, W, max_entries, row_bits);
}

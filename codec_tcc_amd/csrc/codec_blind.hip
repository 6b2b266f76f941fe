// codec_blind.hip -- blind MED-PEE (include/codec_tcc_blind.h; specification:
// tests/pee_blind_spec.py): the planning and the bit plumbing around the ROI embed /
// extract kernels of codec_pee.hip, which do all the prediction-error work unchanged.
//
// Embed, all on one stream, no host round trip:
//   k_blind_rows     one read-only streaming pass, grid (row bands, B), 256 threads.  A wave takes
//                    BL_ROWS_PER_WAVE candidate rows as one run of items (VEC: 8 pixels of a row
//                    pair = 4 candidates, two 16-byte loads (8-byte for uint8), BL_U items in
//                    flight per lane; scalar: one candidate, four loads), keeps one pair of
//                    counters per row in registers, reduces them with shuffles and writes the
//                    rows' (expandable and safe, unsafe) counts.  Plain loads: the cover stays
//                    cached for the embed.  No atomics, no fence, nothing shared between workgroups.
//   k_blind_plan     one workgroup per slice: block scans of the row table, the plan rule, the
//                    arrays codec_pee_roi_embed takes (rectangle, PEE length, T, gate) and info.
//   k_blind_splice   the payload row: displaced LSBs || user bits (a shift by n_side bits).
//   codec_pee_roi_embed on those arrays.
//   k_blind_pack     one workgroup per slice: the map words up to `end` -> ascending entries
//                    (popcount + block scan); header, entries and padding into the stego's LSBs.
// Decode: k_blind_headers (side words 0..5 of every slice, read back once by the host layer),
// then k_blind_zero + k_blind_scatter (entries -> map), codec_pee_roi_extract, k_blind_restore
// (the first n_side extracted bits back into the LSBs, the user bits shifted down).
// Capacity control (include/codec_tcc_blind_auto.h; tests/pee_blind_auto_spec.py): the
// smallest T in 1..tmax whose plan succeeds, per slice, on the device:
//   k_blind_rows_auto  the same pass for every T in 1..16 at once: one classification per candidate
//                    gives its counts at all T as sixteen 4-bit fields of two 64-bit words, summed
//                    per item, widened to bytes and to 16-bit fields in registers, reduced with
//                    shuffles; table [B][tmax][hc].  The cover is read once.
//   k_blind_plan_auto  one workgroup per slice, one wave per T: k_blind_plan's rule with wave scans, the
//                    first T with status 0 (or tmax's refusal), the capacity curve.
// k_blind_splice, the ROI embed and k_blind_pack then run as for a fixed T, on the per-slice T array.
// Keyed (include/codec_tcc_blind_keyed.h; tests/pee_blind_keyed_spec.py): the user stream is
// a 224-bit frame (nonce12, tag) and the ciphertext row.  The plan kernels add the frame's bits to the
// length, k_blind_splice<.., true> reads the stream through the frame (no shifted copy of the row is
// made), k_blind_pack writes the flags it is given; k_blind_frames builds the frames from the ctx block
// and the tags, k_blind_unframe splits the rows k_blind_restore wrote into nonce12, tag and ciphertext.
// Volumes (include/codec_tcc_blind_vol.h; codec_bvol.hip): k_blind_plan_auto, k_blind_scatter
// and k_blind_restore take skip marks (NULL from the entries of this file) -- a marked slice is refused
// with status 3 on the embed side and has no header on the decode side; codec_blind_int.h declares the
// launch sequences codec_bvol.hip puts its plan between and the plan rule's device functions.
// Gated (include/codec_tcc_blind_gate.h; codec_blind_gate.hip): k_blind_pack takes flag bits of
// each slice's own (NULL from the entries of this file), which carry the gate.
// Every kernel clamps what it reads from device memory to the slice, the row and the map.
#include "codec_blind_int.h"
#include "codec_tcc_blind_keyed.h"
#include "codec_tcc_blind_vol.h"

#include <limits.h>

#include <algorithm>

#define BL_PAD 0xFFFFFFFFu
#define BL_ROWS_PER_WAVE 4
#define BL_ROWS_PER_WG (4 * BL_ROWS_PER_WAVE)
#define BL_U 4

// oracle/pee_cpu.py classify: (expandable and safe) + (unsafe << 16) of one candidate
__device__ __forceinline__ uint32_t bl_class(int x, int a, int b, int c, int T, int maxval) {
    const int p = bl_med3(a, b, c), e = x - p;
    const bool expand = (e >= -T) & (e < T);
    const bool safe = expand ? ((p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval)) : (e >= T ? x + T <= maxval : x - T >= 0);
    return ((expand & safe) ? 1u : 0u) + (safe ? 0u : 0x10000u);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_blind_rows(const T* __restrict__ img, int H, int W, int maxval, int thr,
                                                    uint2* __restrict__ rows_out) {
    typedef typename Vec8<T>::type V;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hc = H / 2;
    const int i0 = (int)blockIdx.x * BL_ROWS_PER_WG + wv * BL_ROWS_PER_WAVE;   // the wave's first candidate row
    if (i0 >= hc) return;                                                      // uniform per wave; no barrier below
    const int nrows = min(BL_ROWS_PER_WAVE, hc - i0);
    const T* src = img + (size_t)b * H * W;
    uint32_t acc[BL_ROWS_PER_WAVE] = {0u, 0u, 0u, 0u};   // per row: es + (unsafe << 16); a lane sees < 2^14 of a row
    // a row holds at most 32767 candidates, a lane's share of it at most 512: the halves cannot carry
    if constexpr (VEC) {
        const uint32_t CR = (uint32_t)W / 8;
        const uint32_t n = (uint32_t)nrows * CR;
        for (uint32_t t = (uint32_t)lane; t < n; t += 64u * BL_U) {
            V v0[BL_U], v1[BL_U];
            uint32_t kk[BL_U];
            bool in[BL_U];
#pragma unroll
            for (int u = 0; u < BL_U; ++u) {
                const uint32_t tu = t + 64u * u;
                in[u] = tu < n;
                const uint32_t tc = in[u] ? tu : n - 1u;   // clamped: a valid address
                kk[u] = tc / CR;
                const uint32_t c = tc - kk[u] * CR;
                const size_t o0 = (size_t)(2 * (i0 + (int)kk[u])) * W + (size_t)c * 8;
                v0[u] = *reinterpret_cast<const V*>(src + o0);
                v1[u] = *reinterpret_cast<const V*>(src + o0 + W);
            }
#pragma unroll
            for (int u = 0; u < BL_U; ++u) {
                uint32_t s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    s += bl_class((int)bl_px(v1[u], 2 * q + 1), (int)bl_px(v1[u], 2 * q), (int)bl_px(v0[u], 2 * q + 1),
                                  (int)bl_px(v0[u], 2 * q), thr, maxval);
                s = in[u] ? s : 0u;
#pragma unroll
                for (int k = 0; k < BL_ROWS_PER_WAVE; ++k) acc[k] += kk[u] == (uint32_t)k ? s : 0u;
            }
        }
    } else {
        const uint32_t wc = (uint32_t)W / 2;
        const uint32_t n = (uint32_t)nrows * wc;
        for (uint32_t t = (uint32_t)lane; t < n; t += 64u) {
            const uint32_t k = t / wc, j = t - k * wc;
            const size_t y = 2 * (size_t)(i0 + (int)k) + 1, x = 2 * (size_t)j + 1;
            const uint32_t s = bl_class((int)src[y * W + x], (int)src[y * W + x - 1], (int)src[(y - 1) * W + x],
                                        (int)src[(y - 1) * W + x - 1], thr, maxval);
#pragma unroll
            for (int q = 0; q < BL_ROWS_PER_WAVE; ++q) acc[q] += k == (uint32_t)q ? s : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < BL_ROWS_PER_WAVE; ++k) {
        uint32_t es = acc[k] & 0xFFFFu, un = acc[k] >> 16;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            es += __shfl_xor(es, o, 64);
            un += __shfl_xor(un, o, 64);
        }
        if (lane == 0 && k < nrows) rows_out[(size_t)b * hc + i0 + k] = make_uint2(es, un);
    }
}

// ---- every T in 1..16 from one classification.  A count "for every T > a" is the 64-bit word
// BL_ONES << 4 a: one 4-bit field per T (field T - 1), so that a few candidates add up in place.
#define BL_ONES 0x1111111111111111ull
#define BL_EVEN 0x0F0F0F0F0F0F0F0Full
#define BL_LOW 0x00FF00FF00FF00FFull
#define BL_WIDEN_ITEMS 60   // adds of at most 4 per field before the byte fields are widened: 240 < 256

__device__ __forceinline__ u64 bl_above(int a) { return a < 16 ? BL_ONES << (4 * a) : 0ull; }

// bl_class closed over T: with u = e for e >= 0 and -e - 1 otherwise, the candidate expands iff
// u < T; it is then safe iff ok (no T in that), and otherwise safe iff T <= d, the room towards the
// end of the range it is shifted to.  So: expandable and safe for T > u if ok; unsafe for T > u if
// not ok, and for d < T <= u.
__device__ __forceinline__ void bl_class_all(int x, int a, int b, int c, int maxval, u64& es, u64& un) {
    const int p = bl_med3(a, b, c), e = x - p;
    const int u = e >= 0 ? e : -e - 1;
    const bool ok = (p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval);
    const int d = max(e >= 0 ? maxval - x : x, 0);
    const u64 nu = bl_above(u);
    es += ok ? nu : 0ull;
    un += (ok ? 0ull : nu) + (d < u ? bl_above(d) - nu : 0ull);   // bl_above(u) is a subset of bl_above(d): no borrow
}

// a lane's counts of one candidate row: [0] expandable and safe, [1] unsafe.  by: byte fields,
// [..][0] of T - 1 = 0, 2, .., 14 and [..][1] of 1, 3, .., 15; hf: 16-bit fields, [..][q] of
// T - 1 = BL_HF_FIRST(q) + 4 j in field j.  A lane sees at most 512 candidates of a row.
#define BL_HF_FIRST(q) ((q) == 0 ? 0 : (q) == 1 ? 2 : (q) == 2 ? 1 : 3)
struct BlAcc {
    u64 by[2][2], hf[2][4];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            by[k][0] = by[k][1] = 0ull;
            hf[k][0] = hf[k][1] = hf[k][2] = hf[k][3] = 0ull;
        }
    }
    // es / un: 4-bit fields of at most 4 each
    __device__ __forceinline__ void add(u64 es, u64 un) {
        by[0][0] += es & BL_EVEN; by[0][1] += (es >> 4) & BL_EVEN;
        by[1][0] += un & BL_EVEN; by[1][1] += (un >> 4) & BL_EVEN;
    }
    __device__ __forceinline__ void widen() {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            hf[k][0] += by[k][0] & BL_LOW; hf[k][1] += (by[k][0] >> 8) & BL_LOW;
            hf[k][2] += by[k][1] & BL_LOW; hf[k][3] += (by[k][1] >> 8) & BL_LOW;
            by[k][0] = by[k][1] = 0ull;
        }
    }
    // the wave's sums in every lane: a row has at most 32767 candidates, so no field carries
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t lo = (uint32_t)hf[k][q], hi = (uint32_t)(hf[k][q] >> 32);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    lo += __shfl_xor(lo, o, 64);
                    hi += __shfl_xor(hi, o, 64);
                }
                hf[k][q] = ((u64)hi << 32) | lo;
            }
    }
    // the count of kind k at T = t + 1, t in 0..15
    __device__ __forceinline__ uint32_t at(int k, int t) const {
        const int q = t & 3;
        const u64 w = q == 0 ? hf[k][0] : q == 2 ? hf[k][1] : q == 1 ? hf[k][2] : hf[k][3];
        return (uint32_t)(w >> (16 * (t >> 2))) & 0xFFFFu;
    }
};

// grid and waves as k_blind_rows; a wave takes its candidate rows one after the other, so that a
// row's counts at all T stay in one set of registers.  rows_out: [B][tmax][hc], tmax in 1..16.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_blind_rows_auto(const T* __restrict__ img, int H, int W, int maxval, int tmax,
                                                         uint2* __restrict__ rows_out) {
    typedef typename Vec8<T>::type V;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hc = H / 2;
    const int i0 = (int)blockIdx.x * BL_ROWS_PER_WG + wv * BL_ROWS_PER_WAVE;
    if (i0 >= hc) return;   // uniform per wave; no barrier below
    const int nrows = min(BL_ROWS_PER_WAVE, hc - i0);
    const T* src = img + (size_t)b * H * W;
    for (int k = 0; k < nrows; ++k) {
        BlAcc acc;
        acc.zero();
        int since = 0;
        if constexpr (VEC) {
            const uint32_t CR = (uint32_t)W / 8;
            const T* r0 = src + (size_t)(2 * (i0 + k)) * W;
            for (uint32_t t = (uint32_t)lane; t < CR; t += 64u * BL_U) {
                V v0[BL_U], v1[BL_U];
                bool in[BL_U];
#pragma unroll
                for (int u = 0; u < BL_U; ++u) {
                    const uint32_t tu = t + 64u * u;
                    in[u] = tu < CR;
                    const size_t o0 = (size_t)(in[u] ? tu : CR - 1u) * 8;   // clamped: a valid address
                    v0[u] = *reinterpret_cast<const V*>(r0 + o0);
                    v1[u] = *reinterpret_cast<const V*>(r0 + o0 + W);
                }
#pragma unroll
                for (int u = 0; u < BL_U; ++u) {
                    u64 es = 0ull, un = 0ull;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        bl_class_all((int)bl_px(v1[u], 2 * q + 1), (int)bl_px(v1[u], 2 * q), (int)bl_px(v0[u], 2 * q + 1),
                                     (int)bl_px(v0[u], 2 * q), maxval, es, un);
                    acc.add(in[u] ? es : 0ull, in[u] ? un : 0ull);
                }
                since += BL_U;
                if (since + BL_U > BL_WIDEN_ITEMS) { acc.widen(); since = 0; }
            }
        } else {
            const uint32_t wc = (uint32_t)W / 2;
            const size_t y = 2 * (size_t)(i0 + k) + 1;
            for (uint32_t j = (uint32_t)lane; j < wc; j += 64u) {
                const size_t x = 2 * (size_t)j + 1;
                u64 es = 0ull, un = 0ull;
                bl_class_all((int)src[y * W + x], (int)src[y * W + x - 1], (int)src[(y - 1) * W + x],
                             (int)src[(y - 1) * W + x - 1], maxval, es, un);
                acc.add(es, un);
                if (++since == BL_WIDEN_ITEMS) { acc.widen(); since = 0; }
            }
        }
        acc.widen();
        acc.reduce();
        if (lane < tmax) rows_out[((size_t)b * tmax + lane) * hc + i0 + k] = make_uint2(acc.at(0, lane), acc.at(1, lane));
    }
}

// the plan rule over one slice's row table at one T (rows: its hc entries), by all 256 threads of a
// workgroup, every one of which gets the result.  An entry is clamped to the row's W / 2 candidates.
__device__ BlPlan bl_plan_rows(const uint2* __restrict__ rows, int hc, long long n_user, int W, int max_entries,
                               long long row_bits, uint32_t* sh, u64* s_first, int* s_cap) {
    const int tid = threadIdx.x;
    const uint32_t wc = (uint32_t)W / 2;
    if (tid == 0) { *s_first = ~0ull; *s_cap = -1; }
    __syncthreads();
    uint32_t cap0 = 0, uns0 = 0;
    for (int c0 = 0; c0 < hc; c0 += 256) {
        const int i = c0 + tid;
        uint2 v = i < hc ? rows[i] : make_uint2(0u, 0u);
        v.x = min(v.x, wc);
        v.y = min(v.y, wc);
        uint32_t tc, tu;
        const uint32_t cap = cap0 + block_excl_scan<256>(v.x, sh, &tc) + v.x;   // through row i
        const uint32_t uns = uns0 + block_excl_scan<256>(v.y, sh, &tu) + v.y;
        if (i < hc) {
            const BlRow r = bl_plan_row(cap, uns, W);
            const int c = bl_plan_cap(r, i, uns, hc, max_entries, row_bits);
            if (c >= 0) atomicMax(s_cap, c);
            if (r.room >= n_user) atomicMin(s_first, ((u64)(uint32_t)i << 32) | uns);
        }
        cap0 += tc;
        uns0 += tu;
    }
    __syncthreads();
    return bl_plan_decide(*s_first, *s_cap, hc, n_user, W, max_entries, row_bits);
}

// one workgroup per slice
__global__ __launch_bounds__(256) void k_blind_plan(const uint2* __restrict__ rows, const int32_t* __restrict__ lengths,
                                                    int user_bits, int frame_bits, int H, int W, int thr, int max_entries,
                                                    long long row_bits, int32_t* __restrict__ info,
                                                    int32_t* __restrict__ rect, int32_t* __restrict__ lens,
                                                    int32_t* __restrict__ ts, int32_t* __restrict__ gs) {
    __shared__ uint32_t sh[256 / 64 + 1];
    __shared__ u64 s_first;
    __shared__ int s_cap;
    const int b = blockIdx.x;
    const int hc = H / 2;
    const long long n_user = bl_n_user(lengths, b, user_bits, frame_bits);
    const BlPlan p = bl_plan_rows(rows + (size_t)b * hc, hc, n_user, W, max_entries, row_bits, sh, &s_first, &s_cap);
    if (threadIdx.x == 0) bl_plan_write(b, p, n_user, thr, p.cap, H, W, info, rect, lens, ts, gs);
}

// one workgroup of sixteen waves per slice, wave T - 1 the plan at T over its part of the table
// [B][tmax][hc].  The slice takes the first T whose plan has status 0, else the refusal of tmax
// (t_out 0); info's last word is the largest capacity over the T's, curve (or NULL) [B][tmax] holds each.
// skip (or NULL): a slice with a nonzero entry is refused with status CODEC_PEE_BLIND_SKIPPED and no bits
// (codec_tcc_blind_vol.h: the volume plan gave it none).
__global__ __launch_bounds__(64 * CODEC_PEE_BLIND_TMAX) void k_blind_plan_auto(
    const uint2* __restrict__ rows, const int32_t* __restrict__ lengths, const int32_t* __restrict__ skip, int user_bits,
    int frame_bits, int H, int W,
    int tmax, int max_entries, long long row_bits, int32_t* __restrict__ info, int32_t* __restrict__ t_out,
    int32_t* __restrict__ curve, int32_t* __restrict__ rect, int32_t* __restrict__ lens, int32_t* __restrict__ ts,
    int32_t* __restrict__ gs) {
    __shared__ BlPlan s_plan[CODEC_PEE_BLIND_TMAX];
    const int b = blockIdx.x, wv = threadIdx.x >> 6;
    const int hc = H / 2;
    const long long n_user = bl_n_user(lengths, b, user_bits, frame_bits);
    tmax = min(max(tmax, 1), CODEC_PEE_BLIND_TMAX);
    if (wv < tmax) {
        const BlPlan p = bl_plan_rows_wave(rows + ((size_t)b * tmax + wv) * hc, hc, n_user, W, max_entries, row_bits);
        if ((threadIdx.x & 63) == 0) s_plan[wv] = p;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int tstar = 0, cap = -1;
    for (int T = tmax; T >= 1; --T) {
        cap = max(cap, s_plan[T - 1].cap);
        if (s_plan[T - 1].status == 0) tstar = T;
        if (curve) curve[(size_t)b * tmax + (T - 1)] = s_plan[T - 1].cap;
    }
    if (skip && skip[b]) {
        const BlPlan p = {CODEC_PEE_BLIND_SKIPPED, 0, 0, -1, 0, cap};
        bl_plan_write(b, p, 0, tmax, cap, H, W, info, rect, lens, ts, gs);
        t_out[b] = 0;
        return;
    }
    bl_plan_write(b, s_plan[(tstar ? tstar : tmax) - 1], n_user, tstar ? tstar : tmax, cap, H, W, info, rect, lens, ts, gs);
    t_out[b] = tstar;
}

// word k of slice b's user row, bits past n_user cleared
__device__ __forceinline__ u64 bl_user_word(const u64* __restrict__ row, long long k, long long n_user) {
    const long long nw = (n_user + 63) >> 6;
    if (k < 0 || k >= nw) return 0ull;
    u64 v = row[k];
    const int tail = (int)(n_user & 63);
    if (k == nw - 1 && tail) v &= (1ull << tail) - 1ull;
    return v;
}

// word k of a keyed slice's user stream (codec_tcc_blind_keyed.h): the frame's seven 32-bit words f,
// then the ciphertext row ct, 32 bits off a word; bits past n_user (frame included) cleared
__device__ __forceinline__ u64 bl_keyed_word(const u64* __restrict__ ct, int ct_words, const uint32_t* __restrict__ f,
                                             long long k, long long n_user) {
    const long long nw = (n_user + 63) >> 6;
    if (k < 0 || k >= nw) return 0ull;
    const long long n_ct = min(max(n_user - CODEC_PEE_BLIND_FRAME_BITS, 0LL), 64LL * ct_words);
    u64 v;
    if (k < 3) v = (u64)f[2 * k] | ((u64)f[2 * k + 1] << 32);
    else if (k == 3) v = (u64)f[6] | (bl_user_word(ct, 0, n_ct) << 32);
    else v = (bl_user_word(ct, k - 4, n_ct) >> 32) | (bl_user_word(ct, k - 3, n_ct) << 32);
    const int tail = (int)(n_user & 63);
    if (k == nw - 1 && tail) v &= (1ull << tail) - 1ull;
    return v;
}

// payload row = displaced LSBs (side bit i = bit 0 of pixel npx - 1 - i) || user bits; grid (row words / 256, B).
// KEYED: the user bits are frames[b] || user[b] (bl_keyed_word), info's n_user counting both.
template <typename T, bool KEYED>
__global__ __launch_bounds__(256) void k_blind_splice(const T* __restrict__ img, long long npx,
                                                      const u64* __restrict__ user, int user_words,
                                                      const uint32_t* __restrict__ frames,
                                                      const int32_t* __restrict__ info, u64* __restrict__ out,
                                                      int row_words) {
    const int b = blockIdx.y;
    const int w = (int)blockIdx.x * 256 + threadIdx.x;
    if (w >= row_words) return;
    const int32_t* I = info + (size_t)b * CODEC_PEE_BLIND_INFO_WORDS;
    u64 v = 0;
    if (I[0] == 0) {
        const long long n_user = I[1], n_side = min((long long)I[3], npx);
        const long long lo = 64LL * w;
        const T* src = img + (size_t)b * npx;
        if (lo < n_side)
            for (int j = 0; j < 64; ++j)
                if (lo + j < n_side) v |= (u64)(src[npx - 1 - (lo + j)] & 1) << j;
        if (lo + 64 > n_side && n_user > 0) {
            const u64* row = user + (size_t)b * user_words;
            auto word = [&](long long k) -> u64 {
                if constexpr (KEYED)
                    return bl_keyed_word(row, user_words, frames + (size_t)b * CODEC_PEE_BLIND_FRAME_WORDS, k, n_user);
                else
                    return bl_user_word(row, k, n_user);
            };
            const long long q = lo - n_side;   // the user bit at position lo (negative: the row's first user bit lies inside)
            if (q >= 0) {
                const int sh = (int)(q & 63);
                v |= word(q >> 6) >> sh;
                if (sh) v |= word((q >> 6) + 1) << (64 - sh);
            } else {
                v |= word(0) << (int)(-q);
            }
        }
    }
    out[(size_t)b * row_words + w] = v;
}

template <typename T>
__device__ __forceinline__ void bl_put_word(T* __restrict__ px, long long npx, long long first_bit, uint32_t word) {
    if (first_bit + 32 > npx) return;
    for (int j = 0; j < 32; ++j) {
        T* p = px + (npx - 1 - (first_bit + j));
        *p = (T)((*p & (T)~(T)1) | (T)((word >> j) & 1u));
    }
}
template <typename T>
__device__ __forceinline__ uint32_t bl_get_word(const T* __restrict__ px, long long npx, long long first_bit) {
    if (first_bit + 32 > npx) return 0u;
    uint32_t w = 0;
    for (int j = 0; j < 32; ++j) w |= (uint32_t)(px[npx - 1 - (first_bit + j)] & 1) << j;
    return w;
}

// one workgroup per slice, after the ROI embed: header, entries, padding; info's `end`.  ts: the
// plan's T per slice (clamped to the header's 1..64); flags: the header's (word 5 is crc[b] when they
// have CODEC_PEE_BLIND_FLAG_CRC and crc is given, else 0); flags_b (or NULL): flag bits of each slice's
// own, or-ed in (codec_tcc_blind_gate.h: the gate)
template <typename T>
__global__ __launch_bounds__(256) void k_blind_pack(T* __restrict__ stego, long long npx, int nc,
                                                    const int32_t* __restrict__ ts, int maxval,
                                                    const codec_pee_meta* __restrict__ meta, const u64* __restrict__ lm,
                                                    int lm_words, const uint32_t* __restrict__ crc, uint32_t flags,
                                                    const uint32_t* __restrict__ flags_b, int32_t* __restrict__ info) {
    __shared__ uint32_t sh[256 / 64 + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* I = info + (size_t)b * CODEC_PEE_BLIND_INFO_WORDS;
    if (I[0] != 0) return;   // refused: the ROI embed copied the cover through (length 0, no rectangle)
    const int E = I[2];
    const int end = min(max(meta[b].end, -1), min(nc, 64 * lm_words) - 1);
    T* px = stego + (size_t)b * npx;
    if (tid < CODEC_PEE_BLIND_HDR_WORDS) {
        const int thr = min(max(ts[b], 1), 64);
        if (flags_b) flags |= flags_b[b];
        const uint32_t hw[CODEC_PEE_BLIND_HDR_WORDS] = {
            CODEC_PEE_BLIND_MAGIC,
            (uint32_t)thr | ((flags & 0xFFu) << 8) | ((uint32_t)maxval << 16),
            (uint32_t)I[1], (uint32_t)E, (uint32_t)end, (crc && (flags & CODEC_PEE_BLIND_FLAG_CRC)) ? crc[b] : 0u};
        bl_put_word(px, npx, 32LL * tid, hw[tid]);
    }
    const int nwords = (end + 64) >> 6;   // 0 for end = -1
    uint32_t carry = 0;
    for (int c0 = 0; c0 < nwords; c0 += 256) {
        const int w = c0 + tid;
        u64 m = w < nwords ? lm[(size_t)b * lm_words + w] : 0ull;
        if (w == nwords - 1 && ((end + 1) & 63)) m &= (1ull << ((end + 1) & 63)) - 1ull;
        uint32_t tot;
        uint32_t e = carry + block_excl_scan<256>((uint32_t)__popcll(m), sh, &tot);
        while (m) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            if (e < (uint32_t)E) bl_put_word(px, npx, BL_HDR_BITS + 32LL * e, (uint32_t)(64 * w + bit));
            ++e;
        }
        carry += tot;
    }
    for (uint32_t e = carry + (uint32_t)tid; e < (uint32_t)E; e += 256u) bl_put_word(px, npx, BL_HDR_BITS + 32LL * e, BL_PAD);
    if (tid == 0) I[4] = end;
}

// side words 0 .. 5 of every slice, then two zeros: one thread per output word
template <typename T>
__global__ __launch_bounds__(256) void k_blind_headers(const T* __restrict__ stego, long long npx, int B,
                                                       uint32_t* __restrict__ hdr) {
    const int t = (int)blockIdx.x * 256 + threadIdx.x;
    if (t >= 8 * B) return;
    const int b = t >> 3, k = t & 7;
    hdr[t] = k < CODEC_PEE_BLIND_HDR_WORDS ? bl_get_word(stego + (size_t)b * npx, npx, 32LL * k) : 0u;
}

__global__ __launch_bounds__(256) void k_blind_zero(u64* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0ull;
}

// the header's E and n_side as a decode kernel takes them: clamped to the slice and the row
struct BlHdr {
    long long n_side, n_user;
    int E, end;
};
__device__ __forceinline__ BlHdr bl_hdr(const uint32_t* __restrict__ hdr, int b, long long npx, long long row_bits, int nc) {
    BlHdr h;
    const long long emax = max(0LL, (min(npx, row_bits) - BL_HDR_BITS) / 32);
    h.E = (int)min((long long)hdr[8 * b + 3], emax);
    h.n_side = min((long long)BL_HDR_BITS + 32LL * h.E, min(npx, row_bits));
    h.n_user = min((long long)hdr[8 * b + 2], row_bits - h.n_side);
    const uint32_t e = hdr[8 * b + 4];
    h.end = e == BL_PAD ? -1 : (int)min(e, (uint32_t)(nc - 1));
    return h;
}

// entries -> map bits; grid (entries / 256, B)
template <typename T>
__global__ __launch_bounds__(256) void k_blind_scatter(const T* __restrict__ stego, long long npx, int nc,
                                                       long long row_bits, const uint32_t* __restrict__ hdr,
                                                       const int32_t* __restrict__ skip, u64* __restrict__ lm,
                                                       int lm_words) {
    const int b = blockIdx.y;
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (skip && skip[b]) return;   // no header (codec_tcc_blind_vol.h)
    const BlHdr h = bl_hdr(hdr, b, npx, row_bits, nc);
    if (e >= h.E) return;
    const uint32_t idx = bl_get_word(stego + (size_t)b * npx, npx, BL_HDR_BITS + 32LL * e);
    if (idx == BL_PAD || (long long)idx > (long long)h.end || idx >= (uint32_t)nc || (idx >> 6) >= (uint32_t)lm_words) return;
    atomicOr(reinterpret_cast<u64*>(lm) + (size_t)b * lm_words + (idx >> 6), 1ull << (idx & 63));
}

// after the ROI extract: thread t restores side bit t and writes user word t; grid (max(bits, words) / 256, B).
// skip (or NULL): a slice with a nonzero entry has no side bits and a zero user row.
template <typename T>
__global__ __launch_bounds__(256) void k_blind_restore(T* __restrict__ cover, long long npx, int nc, long long row_bits,
                                                       const uint32_t* __restrict__ hdr, const int32_t* __restrict__ skip,
                                                       const u64* __restrict__ rows, int row_words, u64* __restrict__ out,
                                                       int user_words) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    BlHdr h = bl_hdr(hdr, b, npx, row_bits, nc);
    if (skip && skip[b]) h.n_side = h.n_user = 0;
    const u64* row = rows + (size_t)b * row_words;
    if (t < h.n_side) {
        T* p = cover + (size_t)b * npx + (npx - 1 - t);
        *p = (T)((*p & (T)~(T)1) | (T)((row[t >> 6] >> (t & 63)) & 1ull));
    }
    if (t < user_words) {
        const long long q = h.n_side + 64 * t, k = q >> 6;
        const int s = (int)(q & 63);
        u64 v = k < row_words ? row[k] >> s : 0ull;
        if (s && k + 1 < row_words) v |= row[k + 1] << (64 - s);
        const long long left = h.n_user - 64 * t;   // user bits from this word on
        if (left <= 0) v = 0ull;
        else if (left < 64) v &= (1ull << left) - 1ull;
        out[(size_t)b * user_words + t] = v;
    }
}

// ---- keyed: frames in, frames out (include/codec_tcc_blind_keyed.h)
// one thread per frame word: (index0 + b, the ctx block's nonce words, the slice's tag)
__global__ __launch_bounds__(256) void k_blind_frames(const codec_aead_ctx* __restrict__ ctx, int B, uint32_t index0,
                                                      const uint32_t* __restrict__ tags, uint32_t* __restrict__ frames) {
    const int t = (int)blockIdx.x * 256 + threadIdx.x;
    if (t >= CODEC_PEE_BLIND_FRAME_WORDS * B) return;
    const int b = t / CODEC_PEE_BLIND_FRAME_WORDS, k = t - b * CODEC_PEE_BLIND_FRAME_WORDS;
    frames[t] = k == 0 ? index0 + (uint32_t)b : k < 3 ? ctx->nonce[k - 1] : tags[4 * b + (k - 3)];
}

// the user rows of k_blind_restore -> nonce12, tag, ciphertext rows and lengths; grid (ct words / 256, B).
// Thread t writes ciphertext word t; the first seven threads of a slice also write its frame words.
__global__ __launch_bounds__(256) void k_blind_unframe(const u64* __restrict__ rows, int user_words,
                                                       const uint32_t* __restrict__ hdr, uint32_t* __restrict__ n12,
                                                       uint32_t* __restrict__ tags, u64* __restrict__ ct, int ct_words,
                                                       int32_t* __restrict__ ct_lengths) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const u64* row = rows + (size_t)b * user_words;
    const long long n_user = min((long long)hdr[8 * b + 2], 64LL * user_words);
    const long long n_ct = min(max(n_user - CODEC_PEE_BLIND_FRAME_BITS, 0LL), 64LL * ct_words);
    if (t < CODEC_PEE_BLIND_FRAME_WORDS) {
        const int k = (int)(t >> 1);
        const u64 w = k < user_words ? row[k] : 0ull;
        const uint32_t v = (t & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
        if (t < 3) n12[3 * b + t] = v;
        else tags[4 * b + (t - 3)] = v;
    }
    if (t == 0) ct_lengths[b] = (int32_t)n_ct;
    if (t < ct_words) {
        u64 v = t + 3 < user_words ? row[t + 3] >> 32 : 0ull;
        if (t + 4 < user_words) v |= row[t + 4] << 32;
        const long long left = n_ct - 64 * t;   // ciphertext bits from this word on
        if (left <= 0) v = 0ull;
        else if (left < 64) v &= (1ull << left) - 1ull;
        ct[(size_t)b * ct_words + t] = v;
    }
}

// the checks every entry shares; `ws`: the entry takes the workspace
int blind_check(const codec_pee_params* P, int32_t max_entries, bool ws, size_t* base, const char* who, int32_t tmax) {
    if (!P) return set_err(CODEC_EINVAL, "%s: params is NULL", who);
    if (max_entries < 0 || max_entries > CODEC_PEE_BLIND_MAX_ENTRIES)
        return set_err(CODEC_EINVAL, "%s: max_entries must be in 0..65536", who);
    if (tmax < 1 || tmax > CODEC_PEE_BLIND_TMAX) return set_err(CODEC_EINVAL, "%s: tmax must be in 1..16", who);
    *base = codec_pee_workspace_bytes(P);
    if (!*base) return CODEC_EINVAL;   // codec_pee_workspace_bytes set the text
    int rc = pee_roi_dim_check(P, who);
    if (rc) return rc;
    if (P->T > 64) return set_err(CODEC_EINVAL, "%s: T must be <= 64", who);
    if ((long long)P->H * P->W < BL_HDR_BITS) return set_err(CODEC_EINVAL, "%s: the slice cannot hold the 192 header bits", who);
    if (ws && P->payload_words < CODEC_PEE_BLIND_ROW_WORDS(0, max_entries))
        return set_err(CODEC_EINVAL, "%s: payload_words is below the row of 192 + 32 max_entries side bits", who);
    return 0;
}

// row table and plan on the workspace's arrays (lengths NULL: 0 bits each; frame_bits: bl_n_user)
static int blind_plan(const codec_pee_params* P, const BlWs& L, const void* cover, const int32_t* lengths, int user_bits,
                      int frame_bits, long long row_bits, int32_t max_entries, int32_t* info, char* ws, hipStream_t st) {
    uint2* rows = reinterpret_cast<uint2*>(ws + L.rows);
    const int hc = P->H / 2;
    if (hc > 0) {
        ProfScope prof(st, CODEC_K_BLIND_ROWS);
        dim3 grid((unsigned)((hc + BL_ROWS_PER_WG - 1) / BL_ROWS_PER_WG), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, static_cast<const TT*>(cover), P->H, P->W, P->maxval, P->T, rows);
            };
            pee_flag(pee_vec_route(P, cover), [&](auto v) { go(k_blind_rows<TT, v()>); });
        });
        LAUNCH_CHECK("k_blind_rows");
    }
    hipLaunchKernelGGL(k_blind_plan, dim3((unsigned)P->B), dim3(256), 0, st, rows, lengths, user_bits, frame_bits, P->H,
                       P->W, P->T, (int)max_entries, row_bits, info, reinterpret_cast<int32_t*>(ws + L.rect),
                       reinterpret_cast<int32_t*>(ws + L.lens), reinterpret_cast<int32_t*>(ws + L.ts),
                       reinterpret_cast<int32_t*>(ws + L.gs));
    LAUNCH_CHECK("k_blind_plan");
    return 0;
}

// the table [B][tmax][hc] for every T in 1..tmax: one pass over the cover
int blind_rows_auto(const codec_pee_params* P, const BlWs& L, const void* cover, int32_t tmax, char* ws, hipStream_t st) {
    uint2* rows = reinterpret_cast<uint2*>(ws + L.rows);
    const int hc = P->H / 2;
    if (hc > 0) {
        ProfScope prof(st, CODEC_K_BLIND_ROWS_AUTO);
        dim3 grid((unsigned)((hc + BL_ROWS_PER_WG - 1) / BL_ROWS_PER_WG), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, static_cast<const TT*>(cover), P->H, P->W, P->maxval,
                                   (int)tmax, rows);
            };
            pee_flag(pee_vec_route(P, cover), [&](auto v) { go(k_blind_rows_auto<TT, v()>); });
        });
        LAUNCH_CHECK("k_blind_rows_auto");
    }
    return 0;
}

// the plan that picks T per slice over that table (t_out; curve or NULL; skip or NULL)
int blind_plan_table(const codec_pee_params* P, const BlWs& L, const int32_t* lengths, const int32_t* skip, int user_bits,
                     int frame_bits, long long row_bits, int32_t tmax, int32_t max_entries, int32_t* info, int32_t* t_out,
                     int32_t* curve, char* ws, hipStream_t st) {
    hipLaunchKernelGGL(k_blind_plan_auto, dim3((unsigned)P->B), dim3(64 * CODEC_PEE_BLIND_TMAX), 0, st,
                       reinterpret_cast<const uint2*>(ws + L.rows), lengths, skip, user_bits, frame_bits, P->H, P->W, (int)tmax,
                       (int)max_entries, row_bits, info, t_out, curve, reinterpret_cast<int32_t*>(ws + L.rect),
                       reinterpret_cast<int32_t*>(ws + L.lens), reinterpret_cast<int32_t*>(ws + L.ts),
                       reinterpret_cast<int32_t*>(ws + L.gs));
    LAUNCH_CHECK("k_blind_plan_auto");
    return 0;
}

// both: the pass over the cover, then the plan
static int blind_plan_auto(const codec_pee_params* P, const BlWs& L, const void* cover, const int32_t* lengths,
                           int user_bits, int frame_bits, long long row_bits, int32_t tmax, int32_t max_entries, int32_t* info,
                           int32_t* t_out, int32_t* curve, char* ws, hipStream_t st) {
    int rc = blind_rows_auto(P, L, cover, tmax, ws, st);
    if (rc) return rc;
    return blind_plan_table(P, L, lengths, nullptr, user_bits, frame_bits, row_bits, tmax, max_entries, info, t_out, curve, ws,
                            st);
}

// after a plan: splice, the ROI embed on the plan's arrays, pack.  frames (or NULL): a keyed embed's, the
// user stream being frames[b] || payload[b]; flags: the header's
int blind_embed_planned(const codec_pee_params* P, const BlWs& L, const void* cover, void* stego, const uint64_t* payload,
                        int32_t user_words, const uint32_t* frames, const uint32_t* crc, uint32_t flags, int32_t* info,
                        codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes, void* stream,
                        const uint32_t* flags_b) {
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    u64* rows = reinterpret_cast<u64*>(ws + L.pay);
    const long long npx = (long long)P->H * P->W;
    {
        dim3 grid((unsigned)((P->payload_words + 255) / 256), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, static_cast<const TT*>(cover), npx,
                                   reinterpret_cast<const u64*>(payload), (int)user_words, frames, info, rows, P->payload_words);
            };
            pee_flag(frames != nullptr, [&](auto k) { go(k_blind_splice<TT, k()>); });
        });
        LAUNCH_CHECK("k_blind_splice");
    }
    const int32_t* ts = reinterpret_cast<const int32_t*>(ws + L.ts);
    int rc = codec_pee_roi_embed(P, cover, stego, reinterpret_cast<const uint64_t*>(rows),
                                 reinterpret_cast<const int32_t*>(ws + L.lens), ts, reinterpret_cast<const int32_t*>(ws + L.gs),
                                 reinterpret_cast<const int32_t*>(ws + L.rect), meta, lm, workspace, workspace_bytes, stream);
    if (rc) return rc;
    const int nc = (P->H / 2) * (P->W / 2);
    pee_pixel(P->bytes, [&](auto px) {
        using TT = decltype(px);
        hipLaunchKernelGGL(k_blind_pack<TT>, dim3((unsigned)P->B), dim3(256), 0, st, static_cast<TT*>(stego), npx, nc, ts,
                           P->maxval, meta, reinterpret_cast<const u64*>(lm), P->lm_words, crc, flags, flags_b, info);
    });
    LAUNCH_CHECK("k_blind_pack");
    return 0;
}

// codec_pee_blind_extract behind its checks: zero the map, scatter the entries, the ROI extract, restore
int blind_extract_launch(const codec_pee_params* P, const BlWs& L, const void* stego, const uint32_t* hdr,
                         const codec_pee_meta* meta, const int32_t* skip, void* cover_out, uint64_t* payload_out,
                         int32_t user_words, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    u64* lm = reinterpret_cast<u64*>(ws + L.lm);
    u64* rows = reinterpret_cast<u64*>(ws + L.pay);
    const long long npx = (long long)P->H * P->W, row_bits = 64LL * P->payload_words;
    const int nc = (P->H / 2) * (P->W / 2);
    const size_t nlm = (size_t)P->B * P->lm_words;
    hipLaunchKernelGGL(k_blind_zero, dim3((unsigned)std::min<size_t>(4096, (nlm + 255) / 256)), dim3(256), 0, st, lm, nlm);
    LAUNCH_CHECK("k_blind_zero");
    const long long ebound = (row_bits - BL_HDR_BITS) / 32;   // >= 0 by the row check
    if (ebound > 0) {
        dim3 grid((unsigned)((ebound + 255) / 256), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            hipLaunchKernelGGL(k_blind_scatter<TT>, grid, dim3(256), 0, st, static_cast<const TT*>(stego), npx, nc, row_bits,
                               hdr, skip, lm, P->lm_words);
        });
        LAUNCH_CHECK("k_blind_scatter");
    }
    int rc = codec_pee_roi_extract(P, stego, meta, reinterpret_cast<const uint64_t*>(lm), cover_out,
                               reinterpret_cast<uint64_t*>(rows), workspace, workspace_bytes, stream);
    if (rc) return rc;
    {
        const long long n = std::max(row_bits, (long long)user_words);
        dim3 grid((unsigned)((n + 255) / 256), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            hipLaunchKernelGGL(k_blind_restore<TT>, grid, dim3(256), 0, st, static_cast<TT*>(cover_out), npx, nc, row_bits, hdr,
                               skip, rows, P->payload_words, reinterpret_cast<u64*>(payload_out), (int)user_words);
        });
        LAUNCH_CHECK("k_blind_restore");
    }
    return 0;
}

extern "C" {

size_t codec_pee_blind_workspace_bytes(const codec_pee_params* P, int32_t max_entries) {
    size_t base = 0;
    if (blind_check(P, max_entries, true, &base, "codec_pee_blind_workspace_bytes")) return 0;
    return bl_ws(P, base).total;
}

int codec_pee_blind_plan(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t max_entries,
                         int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    size_t base = 0;
    int rc = blind_check(P, max_entries, true, &base, "codec_pee_blind_plan");
    if (rc) return rc;
    if (!cover || !info || !workspace) return set_err(CODEC_EINVAL, "codec_pee_blind_plan: NULL pointer argument");
    const BlWs L = bl_ws(P, base);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "codec_pee_blind_plan: workspace too small");
    // the registry, as every workspace-taking call: the arrays lie behind THIS shape's layout, so on a
    // workspace in use for a larger shape they fall inside that shape's state
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    // no row is filled here: the plan and the capacity are the format's own, unbounded by a row width
    return blind_plan(P, L, cover, lengths, INT_MAX, 0, 1LL << 40, max_entries, info, static_cast<char*>(workspace),
                      as_stream(stream));
}

int codec_pee_blind_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                          int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t max_entries,
                          int32_t* info, codec_pee_meta* meta, uint64_t* lm, void* workspace, size_t workspace_bytes,
                          void* stream) {
    size_t base = 0;
    int rc = blind_check(P, max_entries, true, &base, "codec_pee_blind_embed");
    if (rc) return rc;
    if (!cover || !stego || !payload || !lengths || !info || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "codec_pee_blind_embed: NULL pointer argument");
    if (cover == stego) return set_err(CODEC_EINVAL, "codec_pee_blind_embed: out of place only (cover == stego)");
    if (user_words < 1 || user_words > (1 << 24)) return set_err(CODEC_EINVAL, "codec_pee_blind_embed: user_words must be in 1..2^24");
    const BlWs L = bl_ws(P, base);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "codec_pee_blind_embed: workspace too small");
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    if ((rc = blind_plan(P, L, cover, lengths, 64 * user_words, 0, 64LL * P->payload_words, max_entries, info,
                         static_cast<char*>(workspace), as_stream(stream))))
        return rc;
    return blind_embed_planned(P, L, cover, stego, payload, user_words, nullptr, crc, crc ? CODEC_PEE_BLIND_FLAG_CRC : 0u, info,
                               meta, lm, workspace, workspace_bytes, stream);
}

int codec_pee_blind_headers(const codec_pee_params* P, const void* stego, uint32_t* hdr_out, void* stream) {
    size_t base = 0;
    int rc = blind_check(P, 0, false, &base, "codec_pee_blind_headers");
    if (rc) return rc;
    if (!stego || !hdr_out) return set_err(CODEC_EINVAL, "codec_pee_blind_headers: NULL pointer argument");
    hipStream_t st = as_stream(stream);
    const long long npx = (long long)P->H * P->W;
    const dim3 grid((unsigned)((8LL * P->B + 255) / 256));
    pee_pixel(P->bytes, [&](auto px) {
        using TT = decltype(px);
        hipLaunchKernelGGL(k_blind_headers<TT>, grid, dim3(256), 0, st, static_cast<const TT*>(stego), npx, P->B, hdr_out);
    });
    LAUNCH_CHECK("k_blind_headers");
    return 0;
}

int codec_pee_blind_extract(const codec_pee_params* P, const void* stego, const uint32_t* hdr,
                            const codec_pee_meta* meta, void* cover_out, uint64_t* payload_out, int32_t user_words,
                            void* workspace, size_t workspace_bytes, void* stream) {
    size_t base = 0;
    int rc = blind_check(P, 0, true, &base, "codec_pee_blind_extract");
    if (rc) return rc;
    if (!stego || !hdr || !meta || !cover_out || !payload_out || !workspace)
        return set_err(CODEC_EINVAL, "codec_pee_blind_extract: NULL pointer argument");
    if (stego == cover_out) return set_err(CODEC_EINVAL, "codec_pee_blind_extract: out of place only (stego == cover_out)");
    if (user_words < 1 || user_words > (1 << 24)) return set_err(CODEC_EINVAL, "codec_pee_blind_extract: user_words must be in 1..2^24");
    const BlWs L = bl_ws(P, base);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "codec_pee_blind_extract: workspace too small");
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    return blind_extract_launch(P, L, stego, hdr, meta, nullptr, cover_out, payload_out, user_words, workspace, workspace_bytes,
                                stream);
}

// ---- include/codec_tcc_blind_auto.h
size_t codec_pee_blind_auto_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries) {
    size_t base = 0;
    if (blind_check(P, max_entries, true, &base, "codec_pee_blind_auto_workspace_bytes", tmax)) return 0;
    return bl_ws(P, base, tmax).total;
}

int codec_pee_blind_plan_auto(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t tmax,
                              int32_t max_entries, int32_t* info, int32_t* t_out, int32_t* curve, void* workspace,
                              size_t workspace_bytes, void* stream) {
    size_t base = 0;
    int rc = blind_check(P, max_entries, true, &base, "codec_pee_blind_plan_auto", tmax);
    if (rc) return rc;
    if (!cover || !info || !t_out || !workspace) return set_err(CODEC_EINVAL, "codec_pee_blind_plan_auto: NULL pointer argument");
    const BlWs L = bl_ws(P, base, tmax);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "codec_pee_blind_plan_auto: workspace too small");
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    return blind_plan_auto(P, L, cover, lengths, INT_MAX, 0, 1LL << 40, tmax, max_entries, info, t_out, curve,
                           static_cast<char*>(workspace), as_stream(stream));
}

int codec_pee_blind_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                               int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t tmax,
                               int32_t max_entries, int32_t* info, int32_t* t_out, codec_pee_meta* meta, uint64_t* lm,
                               void* workspace, size_t workspace_bytes, void* stream) {
    size_t base = 0;
    int rc = blind_check(P, max_entries, true, &base, "codec_pee_blind_embed_auto", tmax);
    if (rc) return rc;
    if (!cover || !stego || !payload || !lengths || !info || !t_out || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "codec_pee_blind_embed_auto: NULL pointer argument");
    if (cover == stego) return set_err(CODEC_EINVAL, "codec_pee_blind_embed_auto: out of place only (cover == stego)");
    if (user_words < 1 || user_words > (1 << 24))
        return set_err(CODEC_EINVAL, "codec_pee_blind_embed_auto: user_words must be in 1..2^24");
    const BlWs L = bl_ws(P, base, tmax);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "codec_pee_blind_embed_auto: workspace too small");
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    if ((rc = blind_plan_auto(P, L, cover, lengths, 64 * user_words, 0, 64LL * P->payload_words, tmax, max_entries, info, t_out,
                              nullptr, static_cast<char*>(workspace), as_stream(stream))))
        return rc;
    return blind_embed_planned(P, L, cover, stego, payload, user_words, nullptr, crc, crc ? CODEC_PEE_BLIND_FLAG_CRC : 0u, info,
                               meta, lm, workspace, workspace_bytes, stream);
}

// ---- include/codec_tcc_blind_keyed.h
int codec_pee_blind_frames(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint32_t* tags,
                           uint32_t* frames_out, void* stream) {
    if (B < 1) return set_err(CODEC_EINVAL, "codec_pee_blind_frames: bad batch B=%d", B);
    if (!(index0 == CODEC_AEAD_STREAM_INDEX && B == 1) && (u64)index0 + (u64)B > (1ull << 31))
        return set_err(CODEC_EINVAL, "codec_pee_blind_frames: slice indices %u .. %llu are not all < 2^31", index0,
                       (u64)index0 + (u64)B - 1);
    if (!ctx || !tags || !frames_out) return set_err(CODEC_EINVAL, "codec_pee_blind_frames: NULL pointer argument");
    const long long n = (long long)CODEC_PEE_BLIND_FRAME_WORDS * B;
    hipLaunchKernelGGL(k_blind_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), ctx, (int)B, index0,
                       tags, frames_out);
    LAUNCH_CHECK("k_blind_frames");
    return 0;
}

int codec_pee_blind_embed_keyed(const codec_pee_params* P, const void* cover, void* stego, const uint32_t* frames,
                                const uint64_t* ct_rows, int32_t ct_words, const int32_t* lengths, int32_t tmax,
                                int32_t max_entries, int32_t* info, int32_t* ts, codec_pee_meta* meta, uint64_t* lm,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_embed_keyed";
    if (P && max_entries >= 0 && max_entries <= CODEC_PEE_BLIND_MAX_ENTRIES && (tmax < 0 || tmax > CODEC_PEE_BLIND_TMAX))
        return set_err(CODEC_EINVAL, "%s: tmax must be in 0..16 (0: the fixed T)", who);
    size_t base = 0;
    int rc = blind_check(P, max_entries, true, &base, who, tmax ? tmax : 1);
    if (rc) return rc;
    if (P->payload_words < CODEC_PEE_BLIND_ROW_WORDS(CODEC_PEE_BLIND_FRAME_BITS, max_entries))
        return set_err(CODEC_EINVAL, "%s: payload_words is below the row of the side bits and the 224 frame bits", who);
    if (!cover || !stego || !frames || !ct_rows || !lengths || !info || (tmax && !ts) || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    if (cover == stego) return set_err(CODEC_EINVAL, "%s: out of place only (cover == stego)", who);
    if (ct_words < 1 || ct_words > (1 << 24)) return set_err(CODEC_EINVAL, "%s: ct_words must be in 1..2^24", who);
    const BlWs L = bl_ws(P, base, tmax ? tmax : 1);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    const long long row_bits = 64LL * P->payload_words;
    const int fb = CODEC_PEE_BLIND_FRAME_BITS;
    char* ws = static_cast<char*>(workspace);
    rc = tmax ? blind_plan_auto(P, L, cover, lengths, 64 * ct_words, fb, row_bits, tmax, max_entries, info, ts, nullptr, ws,
                                as_stream(stream))
              : blind_plan(P, L, cover, lengths, 64 * ct_words, fb, row_bits, max_entries, info, ws, as_stream(stream));
    if (rc) return rc;
    return blind_embed_planned(P, L, cover, stego, ct_rows, ct_words, frames, nullptr, CODEC_PEE_BLIND_FLAG_KEYED, info, meta,
                               lm, workspace, workspace_bytes, stream);
}

int codec_pee_blind_unframe(int32_t B, const uint64_t* rows, int32_t user_words, const uint32_t* hdr,
                            uint32_t* nonce12_out, uint32_t* tags_out, uint64_t* ct_out, int32_t ct_words,
                            int32_t* ct_lengths_out, void* stream) {
    if (B < 1 || B > 65535) return set_err(CODEC_EINVAL, "codec_pee_blind_unframe: bad batch B=%d (1..65535)", B);
    if (user_words < 1 || user_words > (1 << 24) || ct_words < 1 || ct_words > (1 << 24))
        return set_err(CODEC_EINVAL, "codec_pee_blind_unframe: user_words and ct_words must be in 1..2^24");
    if (!rows || !hdr || !nonce12_out || !tags_out || !ct_out || !ct_lengths_out)
        return set_err(CODEC_EINVAL, "codec_pee_blind_unframe: NULL pointer argument");
    dim3 grid((unsigned)((ct_words + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(k_blind_unframe, grid, dim3(256), 0, as_stream(stream), reinterpret_cast<const u64*>(rows),
                       (int)user_words, hdr, nonce12_out, tags_out, reinterpret_cast<u64*>(ct_out), (int)ct_words,
                       ct_lengths_out);
    LAUNCH_CHECK("k_blind_unframe");
    return 0;
}

}  // extern "C"

// codec_blind_gate.hip -- gated blind MED-PEE (include/codec_tcc_blind_gate.h; specification:
// tests/pee_blind_gate_spec.py): the pass and the plan that choose (T, gate) per slice.  The
// splice, the ROI embed and the pack are codec_blind.hip's (blind_embed_planned), the decode is unchanged.
//
//   k_blind_rows_gate  one read-only streaming pass with k_blind_rows_auto's grid, routes and loads (grid
//                    (row bands, B), 256 threads, a wave takes BLG_ROWS_PER_WAVE candidate rows one after
//                    the other; VEC: 8 pixels of a row pair = 4 candidates, two 16-byte loads (8-byte for
//                    uint8), BLG_U items in flight per lane; scalar: one candidate, four loads).  Plain
//                    loads: the cover stays cached for the embed.  A candidate is classified once: its
//                    roughness class j (closed form, no table) and, closed over T as bl_class_all, the
//                    folded error u, ok and the room d.  Its counts at every T are two step functions of
//                    T, so it goes into a wave-private LDS histogram of the row as at most three updates:
//                    es[j][u] += 1 (expandable and safe for T > u), and the unsafe counts as differences
//                    un[j][t] += 1 where they start, -= 1 where they end.  The bins are replicated
//                    BLG_REP times by lane, so that a smooth row, which crowds into a few bins, spreads
//                    over as many banks.  After the row the 64 lanes read the 2 x 16 x 16 bins out (and
//                    zero them), prefix them over T (in the lane, then across the four lane groups) and
//                    over the classes (16-lane shuffles) and write the row's word cap | uns << 16 at
//                    every (T, class <= j): table [B][tmax][16][hc].  No barrier, no global atomic.
//   k_blind_plan_gate  one workgroup of sixteen waves per slice: wave w applies the plan rule
//                    (bl_plan_rows_wave_by) to the pairs w, w + 16, ..; one thread then takes the first
//                    pair in (T, j) order with status 0 among those the call leaves free and writes info,
//                    the chosen pair, the curve, the ROI embed's arrays and the slice's flag bits.
// Every kernel clamps what it reads from device memory to the slice, the row and the ladder.
#include "codec_blind_int.h"
#include "codec_tcc_blind_gate.h"

#define BLG_ROWS_PER_WAVE 4
#define BLG_ROWS_PER_WG (4 * BLG_ROWS_PER_WAVE)
#define BLG_U 4
#define BLG_CLASSES CODEC_PEE_GATE_CLASSES
#define BLG_REP 4                                           // copies of every bin, by lane & 3
#define BLG_KIND (BLG_CLASSES * CODEC_PEE_BLIND_TMAX * BLG_REP)   // words of one kind's bins: [class][t][copy]
#define BLG_WAVE_WORDS (2 * BLG_KIND)                       // es, then un: 2048 words = 8 KB per wave

__constant__ int c_blg_gates[BLG_CLASSES] = {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535};

// the first j with d <= GATES[j], as codec_gate.hip's table pass: j = d for d <= 4; above, with
// x = d - 1, m = floor(log2 x) and s = the bit below x's leading one, j = 1 + 2 m + s up to x = 127
__device__ __forceinline__ int blg_class(int d) {
    const int x = d - 1;
    const int m = 31 - __clz(max(x, 4));
    const int s = (x >> (m - 1)) & 1;
    return d <= 4 ? d : (x >= 128 ? BLG_CLASSES - 1 : 1 + 2 * m + s);
}

__device__ __forceinline__ void blg_inc(int* p, int v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // result unused: no return
}

// the wave's LDS operations so far are performed before those that follow (one wave: no barrier)
__device__ __forceinline__ void blg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one candidate into the wave's bins h (already offset by the lane's copy).  bl_class_all's closed form:
// expandable and safe for T > u if ok; unsafe for T > min(u, d) if not ok, and for d < T <= u if ok.
// Bins from tmax on are never read.
__device__ __forceinline__ void blg_add(int* h, int x, int a, int b, int c, int maxval, int tmax) {
    const int p = bl_med3(a, b, c), e = x - p;
    const int u = e >= 0 ? e : -e - 1;
    const bool ok = (p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval);
    const int d = max(e >= 0 ? maxval - x : x, 0);
    const int j = blg_class(max(max(a, b), c) - min(min(a, b), c));
    int* es = h + j * (CODEC_PEE_BLIND_TMAX * BLG_REP);
    int* un = es + BLG_KIND;
    if (ok) {
        if (u < tmax) blg_inc(es + u * BLG_REP, 1);
        if (d < u && d < tmax) {
            blg_inc(un + d * BLG_REP, 1);
            if (u < tmax) blg_inc(un + u * BLG_REP, -1);
        }
    } else {
        const int m = min(u, d);
        if (m < tmax) blg_inc(un + m * BLG_REP, 1);
    }
}

// rows_out: [B][tmax][16][hc] words cap | uns << 16, tmax in 1..16
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_blind_rows_gate(const T* __restrict__ img, int H, int W, int maxval, int tmax,
                                                         uint32_t* __restrict__ rows_out) {
    typedef typename Vec8<T>::type V;
    __shared__ __attribute__((aligned(16))) int hist[4][BLG_WAVE_WORDS];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hc = H / 2;
    const int i0 = (int)blockIdx.x * BLG_ROWS_PER_WG + wv * BLG_ROWS_PER_WAVE;
    if (i0 >= hc) return;   // uniform per wave; no workgroup barrier below
    const int nrows = min(BLG_ROWS_PER_WAVE, hc - i0);
    const T* src = img + (size_t)b * H * W;
    int* hw = hist[wv];
    int4* hw4 = reinterpret_cast<int4*>(hw);
    for (int w = lane; w < BLG_WAVE_WORDS / 4; w += 64) hw4[w] = make_int4(0, 0, 0, 0);
    blg_wave_sync();
    int* mine = hw + (lane & (BLG_REP - 1));
    const int cls = lane & 15, grp = lane >> 4;   // the read-out: class cls, T - 1 = 4 grp .. 4 grp + 3
    for (int k = 0; k < nrows; ++k) {
        if constexpr (VEC) {
            const uint32_t CR = (uint32_t)W / 8;
            const T* r0 = src + (size_t)(2 * (i0 + k)) * W;
            for (uint32_t t = (uint32_t)lane; t < CR; t += 64u * BLG_U) {
                V v0[BLG_U], v1[BLG_U];
                bool in[BLG_U];
#pragma unroll
                for (int u = 0; u < BLG_U; ++u) {
                    const uint32_t tu = t + 64u * u;
                    in[u] = tu < CR;
                    const size_t o0 = (size_t)(in[u] ? tu : CR - 1u) * 8;   // clamped: a valid address
                    v0[u] = *reinterpret_cast<const V*>(r0 + o0);
                    v1[u] = *reinterpret_cast<const V*>(r0 + o0 + W);
                }
#pragma unroll
                for (int u = 0; u < BLG_U; ++u)
                    if (in[u]) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            blg_add(mine, (int)bl_px(v1[u], 2 * q + 1), (int)bl_px(v1[u], 2 * q), (int)bl_px(v0[u], 2 * q + 1),
                                    (int)bl_px(v0[u], 2 * q), maxval, tmax);
                    }
            }
        } else {
            const uint32_t wc = (uint32_t)W / 2;
            const size_t y = 2 * (size_t)(i0 + k) + 1;
            for (uint32_t j = (uint32_t)lane; j < wc; j += 64u) {
                const size_t x = 2 * (size_t)j + 1;
                blg_add(mine, (int)src[y * W + x], (int)src[y * W + x - 1], (int)src[(y - 1) * W + x],
                        (int)src[(y - 1) * W + x - 1], maxval, tmax);
            }
        }
        blg_wave_sync();
        // read the row's bins out and zero them: the lane's four T of its class, the copies summed
        int es[4], un[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int at = cls * CODEC_PEE_BLIND_TMAX + 4 * grp + q;   // in int4 units: one bin's copies
            const int4 e4 = hw4[at], u4 = hw4[BLG_KIND / 4 + at];
            hw4[at] = make_int4(0, 0, 0, 0);
            hw4[BLG_KIND / 4 + at] = make_int4(0, 0, 0, 0);
            es[q] = e4.x + e4.y + e4.z + e4.w;
            un[q] = u4.x + u4.y + u4.z + u4.w;
        }
        blg_wave_sync();
        // prefix over T: in the lane, then the totals of the lane groups below
#pragma unroll
        for (int q = 1; q < 4; ++q) { es[q] += es[q - 1]; un[q] += un[q - 1]; }
        int oe = 0, ou = 0;
#pragma unroll
        for (int g = 1; g < 4; ++g) {
            const int se = __shfl(es[3], lane - 16 * g, 64), su = __shfl(un[3], lane - 16 * g, 64);
            if (grp >= g) { oe += se; ou += su; }
        }
        // a row has at most 32767 candidates: every count and every sum over the classes fits 15 bits
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t w = ((uint32_t)(es[q] + oe) & 0xFFFFu) | (((uint32_t)(un[q] + ou) & 0xFFFFu) << 16);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const uint32_t v = __shfl_up(w, o, 16);
                w += cls >= o ? v : 0u;
            }
            const int t = 4 * grp + q;
            if (t < tmax) rows_out[(((size_t)b * tmax + t) * BLG_CLASSES + cls) * hc + i0 + k] = w;
        }
    }
}

// one workgroup of sixteen waves per slice over the table [B][tmax][16][hc].  t_fixed (0: free) in
// 0..tmax, j_fixed (-1: free) in -1..15; curve (or NULL) [B][tmax][16]; flags_b (or NULL) [B].
__global__ __launch_bounds__(1024) void k_blind_plan_gate(
    const uint32_t* __restrict__ rows, const int32_t* __restrict__ lengths, int user_bits, int H, int W, int tmax, int t_fixed,
    int j_fixed, int max_entries, long long row_bits, int32_t* __restrict__ info, int32_t* __restrict__ t_out,
    int32_t* __restrict__ g_out, int32_t* __restrict__ curve, int32_t* __restrict__ rect, int32_t* __restrict__ lens,
    int32_t* __restrict__ ts, int32_t* __restrict__ gs, uint32_t* __restrict__ flags_b) {
    __shared__ BlPlan s_plan[CODEC_PEE_BLIND_TMAX * BLG_CLASSES];
    const int b = blockIdx.x, wv = threadIdx.x >> 6;
    const int hc = H / 2;
    const long long n_user = bl_n_user(lengths, b, user_bits, 0);
    tmax = min(max(tmax, 1), CODEC_PEE_BLIND_TMAX);
    t_fixed = min(max(t_fixed, 0), tmax);
    j_fixed = min(max(j_fixed, -1), BLG_CLASSES - 1);
    for (int pi = wv; pi < tmax * BLG_CLASSES; pi += 16) {   // uniform per wave
        const uint32_t* tab = rows + ((size_t)b * tmax * BLG_CLASSES + pi) * hc;
        const BlPlan p = bl_plan_rows_wave_by([&](int i) { const uint32_t w = tab[i]; return make_uint2(w & 0xFFFFu, w >> 16); },
                                              hc, n_user, W, max_entries, row_bits);
        if ((threadIdx.x & 63) == 0) s_plan[pi] = p;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int t_lo = t_fixed ? t_fixed : 1, t_hi = t_fixed ? t_fixed : tmax;
    const int j_lo = j_fixed >= 0 ? j_fixed : 0, j_hi = j_fixed >= 0 ? j_fixed : BLG_CLASSES - 1;
    int tstar = 0, jstar = -1, cap = -1;
    for (int T = t_hi; T >= t_lo; --T)
        for (int j = j_hi; j >= j_lo; --j) {   // descending: the last hit is the first pair in (T, j) order
            const BlPlan& p = s_plan[(T - 1) * BLG_CLASSES + j];
            cap = max(cap, p.cap);
            if (p.status == 0) { tstar = T; jstar = j; }
        }
    if (curve)
        for (int pi = 0; pi < tmax * BLG_CLASSES; ++pi) curve[(size_t)b * tmax * BLG_CLASSES + pi] = s_plan[pi].cap;
    const int T = tstar ? tstar : t_hi, j = tstar ? jstar : j_hi;
    bl_plan_write(b, s_plan[(T - 1) * BLG_CLASSES + j], n_user, T, cap, H, W, info, rect, lens, ts, gs, c_blg_gates[j]);
    t_out[b] = tstar;
    g_out[b] = tstar ? c_blg_gates[j] : -1;
    if (flags_b) flags_b[b] = CODEC_PEE_BLIND_FLAG_GATED | ((uint32_t)j << CODEC_PEE_BLIND_FLAG_GATE_SHIFT);
}

// the layout: the blind workspace with the table in the row table's place, then one flag word per slice
struct BlgWs {
    BlWs L;
    size_t flags, total;
};
static BlgWs blg_ws(const codec_pee_params* P, size_t base, int32_t tmax) {
    BlgWs G;
    G.L = bl_ws(P, base, tmax * BLG_CLASSES / 2);   // 4-byte words where bl_ws counts 8-byte pairs
    G.flags = G.L.total;
    G.total = G.flags + align_up((size_t)P->B * 4, 256);
    return G;
}

// the checks the entries share, in the header's order up to the NULL pointers
static int blg_check(const codec_pee_params* P, int32_t tmax, int32_t t_fixed, int32_t j_fixed, int32_t max_entries,
                     size_t* base, const char* who) {
    int rc = blind_check(P, max_entries, true, base, who, tmax);
    if (rc) return rc;
    if (t_fixed < 0 || t_fixed > tmax) return set_err(CODEC_EINVAL, "%s: t_fixed must be in 0..tmax (0: free)", who);
    if (j_fixed < -1 || j_fixed >= BLG_CLASSES) return set_err(CODEC_EINVAL, "%s: j_fixed must be in -1..15 (-1: free)", who);
    return 0;
}

// the pass over the cover, then the plan
static int blg_plan(const codec_pee_params* P, const BlgWs& G, const void* cover, const int32_t* lengths, int user_bits,
                    long long row_bits, int32_t tmax, int32_t t_fixed, int32_t j_fixed, int32_t max_entries, int32_t* info,
                    int32_t* t_out, int32_t* g_out, int32_t* curve, char* ws, hipStream_t st) {
    uint32_t* rows = reinterpret_cast<uint32_t*>(ws + G.L.rows);
    const int hc = P->H / 2;
    if (hc > 0) {
        ProfScope prof(st, CODEC_K_BLIND_ROWS_GATE);
        dim3 grid((unsigned)((hc + BLG_ROWS_PER_WG - 1) / BLG_ROWS_PER_WG), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, static_cast<const TT*>(cover), P->H, P->W, P->maxval,
                                   (int)tmax, rows);
            };
            pee_flag(pee_vec_route(P, cover), [&](auto v) { go(k_blind_rows_gate<TT, v()>); });
        });
        LAUNCH_CHECK("k_blind_rows_gate");
    }
    hipLaunchKernelGGL(k_blind_plan_gate, dim3((unsigned)P->B), dim3(1024), 0, st, rows, lengths, user_bits, P->H, P->W,
                       (int)tmax, (int)t_fixed, (int)j_fixed, (int)max_entries, row_bits, info, t_out, g_out, curve,
                       reinterpret_cast<int32_t*>(ws + G.L.rect), reinterpret_cast<int32_t*>(ws + G.L.lens),
                       reinterpret_cast<int32_t*>(ws + G.L.ts), reinterpret_cast<int32_t*>(ws + G.L.gs),
                       reinterpret_cast<uint32_t*>(ws + G.flags));
    LAUNCH_CHECK("k_blind_plan_gate");
    return 0;
}

extern "C" {

size_t codec_pee_blind_gate_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries) {
    size_t base = 0;
    if (blind_check(P, max_entries, true, &base, "codec_pee_blind_gate_workspace_bytes", tmax)) return 0;
    return blg_ws(P, base, tmax).total;
}

int codec_pee_blind_plan_gate(const codec_pee_params* P, const void* cover, const int32_t* lengths, int32_t tmax,
                              int32_t t_fixed, int32_t j_fixed, int32_t max_entries, int32_t* info, int32_t* t_out,
                              int32_t* g_out, int32_t* curve, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_plan_gate";
    size_t base = 0;
    int rc = blg_check(P, tmax, t_fixed, j_fixed, max_entries, &base, who);
    if (rc) return rc;
    if (!cover || !info || !t_out || !g_out || !workspace) return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    const BlgWs G = blg_ws(P, base, tmax);
    if (workspace_bytes < G.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    // no row is filled here: the plan and the capacity are the format's own, unbounded by a row width
    return blg_plan(P, G, cover, lengths, INT_MAX, 1LL << 40, tmax, t_fixed, j_fixed, max_entries, info, t_out, g_out, curve,
                    static_cast<char*>(workspace), as_stream(stream));
}

int codec_pee_blind_embed_gate(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                               int32_t user_words, const int32_t* lengths, const uint32_t* crc, int32_t tmax,
                               int32_t t_fixed, int32_t j_fixed, int32_t max_entries, int32_t* info, int32_t* t_out,
                               int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_embed_gate";
    size_t base = 0;
    int rc = blg_check(P, tmax, t_fixed, j_fixed, max_entries, &base, who);
    if (rc) return rc;
    if (!cover || !stego || !payload || !lengths || !info || !t_out || !g_out || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    if (cover == stego) return set_err(CODEC_EINVAL, "%s: out of place only (cover == stego)", who);
    if (user_words < 1 || user_words > (1 << 24)) return set_err(CODEC_EINVAL, "%s: user_words must be in 1..2^24", who);
    const BlgWs G = blg_ws(P, base, tmax);
    if (workspace_bytes < G.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    char* ws = static_cast<char*>(workspace);
    if ((rc = blg_plan(P, G, cover, lengths, 64 * user_words, 64LL * P->payload_words, tmax, t_fixed, j_fixed, max_entries, info,
                       t_out, g_out, nullptr, ws, as_stream(stream))))
        return rc;
    return blind_embed_planned(P, G.L, cover, stego, payload, user_words, nullptr, crc, crc ? CODEC_PEE_BLIND_FLAG_CRC : 0u, info,
                               meta, lm, workspace, workspace_bytes, stream, reinterpret_cast<const uint32_t*>(ws + G.flags));
}

}  // extern "C"

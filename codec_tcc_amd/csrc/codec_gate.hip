// codec_gate.hip -- smoothness-gated MED-PEE (include/codec_tcc_gate.h; specification:
// tests/pee_gate_spec.py): the gated capacity table, the (T, G) selection and the entry that
// queues table + selection + embed on one stream.  The gated embed / extract kernels are the
// GATE = true instantiations of codec_pee.hip's (codec_pee_gate_embed / _extract live there).
//
// k_pee_gate_table: one read-only pass, grid (regions, B), 256 threads.  A candidate falls
// into bin (row, j): j = its roughness class (first j with D <= GATES[j]), row = its folded
// error u when the expansion is safe and u < tmax, else row tmax ("the rest": it only counts
// towards n[j]).  That is (tmax + 1) * 16 <= 272 bins per slice, and a smooth slice crowds
// into a handful of them, where same-address LDS atomics run at ~0.5 lane-ops per cycle
// (DESIGN §3).  So the counters are lane-private, as k_pee_ehist's: a workgroup region is
// 4096 items = at most 64 candidates per lane, which fits a byte -- four classes share one
// 32-bit LDS word, word (row * 4 + j / 4) of lane t at index word * 256 + t (a lane always
// hits its own bank), 68 words * 256 lanes * 4 B = 68 KB, sized for tmax = 16 (static: two
// workgroups per CU whatever tmax is).
// A lane's four candidates are merged by word first; an update is then a plain read-add-write.
// Hand-off as k_pee_ehist: the workgroup's bins go to the slice's global bins with returning
// device-scope atomics (waited for before the barrier, so performed before the arrival
// ticket -- no agent-scope fence, which writes back the XCD's L2), and the slice's last
// workgroup reads them with device-scope atomic loads, writes the table out and applies the
// selection rule in 64-bit integer arithmetic.  The bins are zeroed by a small launch before the
// pass (k_pee_gate_zero): the tail of the workspace carries nothing from call to call.
#include "codec_common.h"
#include "codec_tcc_gate.h"
#include "codec_tcc_roi.h"

#define GT_CLASSES CODEC_PEE_GATE_CLASSES
#define GT_TMAX CODEC_PEE_GATE_TMAX
#define GT_BINS ((GT_TMAX + 1) * GT_CLASSES)   // per slice, in the workspace (any tmax)
#define GT_PER_WG 4096                         // items (or candidates) per workgroup: <= 64 per lane

__device__ __forceinline__ int gt_med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), a + b - c)); }

template <typename V> __device__ __forceinline__ uint32_t gt_px(const V& v, int e);
template <> __device__ __forceinline__ uint32_t gt_px<uint4>(const uint4& v, int e) {
    const uint32_t w = e < 2 ? v.x : (e < 4 ? v.y : (e < 6 ? v.z : v.w));
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
template <> __device__ __forceinline__ uint32_t gt_px<uint2>(const uint2& v, int e) {
    return ((e < 4 ? v.x : v.y) >> (8 * (e & 3))) & 0xFFu;
}

// class of roughness d >= 0 on the ladder 0 1 2 3 4 6 8 12 16 24 32 48 64 96 128 65535: the
// first j with d <= GATES[j].  d <= 4: j = d.  Above, the gates are 2^m and 1.5 * 2^m, so with
// x = d - 1 (d <= g iff x < g), m = floor(log2 x) and s = x's bit below the leading one,
// 2^m (1 + s / 2) <= x < the next gate: j = 5 + 2 (m - 2) + s for 4 <= x < 128, and 15 beyond.
__device__ __forceinline__ int gt_class(int d) {
    const int x = d - 1;
    const int m = 31 - __clz(max(x, 4));
    const int s = (x >> (m - 1)) & 1;
    const int j = 1 + 2 * m + s;
    return d <= 4 ? d : (x >= 128 ? 15 : j);
}

// bin update for the (up to) four candidates of one item: packed byte counters, lane-private.
// which: the first `which` candidates count; MASK (the instantiations with rectangles): bit q of
// `which` set = candidate q counts (it exists and lies outside the slice's rectangle)
template <bool MASK>
__device__ __forceinline__ void gt_add4(uint32_t* cnt, int tid, const int (&x)[4], const int (&a)[4],
                                        const int (&bb)[4], const int (&cc)[4], int which, int tmax, int maxval,
                                        int g_fixed) {
    int ad[4];
    uint32_t inc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = gt_med3(a[q], bb[q], cc[q]), e = x[q] - p;
        const int u = e >= 0 ? e : -e - 1;
        const bool hs = (u < tmax) & (p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval);
        const int row = hs ? u : tmax;
        const int d = max(max(a[q], bb[q]), cc[q]) - min(min(a[q], bb[q]), cc[q]);
        const int j = g_fixed >= 0 ? (d <= g_fixed ? 0 : GT_CLASSES - 1) : gt_class(d);
        ad[q] = (row * 4 + (j >> 2)) * 256 + tid;
        inc[q] = (MASK ? ((which >> q) & 1) != 0 : q < which) ? 1u << (8 * (j & 3)) : 0u;
    }
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < q; ++r) {   // branch-free merge of equal words
            const bool same = (inc[r] != 0u) & (inc[q] != 0u) & (ad[r] == ad[q]);
            inc[r] += same ? inc[q] : 0u;
            inc[q] = same ? 0u : inc[q];
        }
    uint32_t old[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) old[q] = cnt[ad[q]];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (inc[q]) cnt[ad[q]] = old[q] + inc[q];   // masked: a merged duplicate must not write back
}

// the selection rule on one slice's table tbl[(tmax + 1)][16] (LDS; row tmax = the rest)
__device__ void gt_select(const uint32_t* tbl, int tmax, int t_fixed, int g_fixed, u64 L, int32_t* t_out, int32_t* g_out,
                          int32_t* k_out) {
    const int gates[GT_CLASSES] = {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535};
    u64 kc[GT_CLASSES], sc[GT_CLASSES], nn[GT_CLASSES];   // per class: sum of hs / of hs * cost over u < T; n
#pragma unroll
    for (int j = 0; j < GT_CLASSES; ++j) {
        kc[j] = sc[j] = 0ull;
        u64 s = 0;
        for (int r = 0; r <= tmax; ++r) s += tbl[r * GT_CLASSES + j];
        nn[j] = s;
    }
    bool have = false;
    u64 bestA = 0, bestK = 0;
    int bestT = t_fixed > 0 ? t_fixed : tmax, bestJ = GT_CLASSES - 1;
    u64 k_inf = 0;   // K(bestT, 15) of the infeasible default
    for (int T = 1; T <= tmax; ++T) {
        const u64 cost = (u64)((T - 1) * (T - 1) + T * T);
#pragma unroll
        for (int j = 0; j < GT_CLASSES; ++j) {
            const u64 h = tbl[(T - 1) * GT_CLASSES + j];
            kc[j] += h;
            sc[j] += h * cost;
        }
        if (t_fixed > 0 && T != t_fixed) continue;
        u64 K = 0, S = 0, N = 0;
        if (g_fixed >= 0) {   // one column: the smallest T that holds L
            if (!have && kc[0] >= L) { have = true; bestT = T; bestK = kc[0]; }
            k_inf = kc[0];
            continue;
        }
#pragma unroll
        for (int j = 0; j < GT_CLASSES; ++j) {
            K += kc[j]; S += sc[j]; N += nn[j];
            const u64 A = 2ull * (u64)(T * T) * (N - K) + S;
            if (L == 0) {   // nothing to embed: (the first T considered, class 0)
                if (!have) { have = true; bestA = A; bestK = K; bestT = T; bestJ = 0; }
            } else if (K >= L && (!have || A * bestK < bestA * K)) {
                have = true; bestA = A; bestK = K; bestT = T; bestJ = j;
            }
        }
        k_inf = K;
    }
    if (t_out) *t_out = bestT;
    if (g_out) *g_out = g_fixed >= 0 ? g_fixed : gates[bestJ];
    if (k_out) *k_out = (int32_t)(have ? bestK : k_inf);
}

// ROI... roi: nothing, or the slices' rectangles (codec_pee_roi_capacity; codec_common.h, pee_roi_arg)
template <typename T, bool VEC, typename... ROI>
__global__ __launch_bounds__(256) void k_pee_gate_table(const T* __restrict__ img, int H, int W, int maxval, int tmax,
                                                        int t_fixed, int g_fixed, uint32_t* __restrict__ gbins_all,
                                                        uint32_t* __restrict__ arrivals,
                                                        const int32_t* __restrict__ lengths, uint32_t* __restrict__ n_out,
                                                        uint32_t* __restrict__ hs_out, int32_t* __restrict__ t_out,
                                                        int32_t* __restrict__ g_out, int32_t* __restrict__ k_out,
                                                        ROI... roi) {
    typedef typename Vec8<T>::type V;
    __shared__ uint32_t cnt[(GT_TMAX + 1) * 4 * 256];   // [(tmax + 1) * 4][256] packed byte counters: 68 KB
    __shared__ uint32_t bins[GT_BINS];
    __shared__ uint32_t ticket;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nw = (tmax + 1) * 4, nb = (tmax + 1) * GT_CLASSES;
    const T* src = img + (size_t)b * H * W;
    // the slice's rectangle (codec_pee_roi_capacity; NULL: none): protected candidates fall into no class
    constexpr bool HAS_ROI = sizeof...(ROI) != 0;
    const PeeRoi R = pee_roi_arg(b, roi...);
    for (int w = 0; w < nw; ++w) cnt[w * 256 + tid] = 0u;
    for (int i = tid; i < nb; i += 256) bins[i] = 0u;
    __syncthreads();
    if constexpr (VEC) {
        const uint32_t CR = (uint32_t)W / 8;
        const uint32_t items = (uint32_t)(H / 2) * CR;
        const uint32_t i0 = (uint32_t)blockIdx.x * GT_PER_WG;
        const uint32_t i1 = min(items, i0 + GT_PER_WG);
        constexpr int U = 4;   // 4 items per thread per step, their 8 loads issued together
        for (uint32_t it = i0 + (uint32_t)tid; it < i1; it += 256 * U) {
            V v0[U], v1[U];
            bool in[U];
            int okm[U];   // with rectangles: the item's candidates outside its slice's
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const uint32_t ik = it + 256u * k;
                in[k] = ik < i1;
                const uint32_t r = ik / CR, c = ik - r * CR;
                okm[k] = 0;
                if constexpr (HAS_ROI) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) okm[k] |= (in[k] && !pee_roi_in(R, (int)r, (int)(4u * c) + q)) ? 1 << q : 0;
                }
                const size_t o0 = in[k] ? (size_t)(2 * r) * W + (size_t)c * 8 : 0;   // clamped: a valid address
                v0[k] = *reinterpret_cast<const V*>(src + o0);
                v1[k] = *reinterpret_cast<const V*>(src + o0 + W);
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                int x[4], a[4], bb[4], cc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    x[q] = (int)gt_px(v1[k], 2 * q + 1); a[q] = (int)gt_px(v1[k], 2 * q);
                    bb[q] = (int)gt_px(v0[k], 2 * q + 1); cc[q] = (int)gt_px(v0[k], 2 * q);
                }
                gt_add4<HAS_ROI>(cnt, tid, x, a, bb, cc, HAS_ROI ? okm[k] : (in[k] ? 4 : 0), tmax, maxval, g_fixed);
            }
        }
    } else {
        const int wc = W / 2;
        const int nc = (H / 2) * wc;
        const int k0 = blockIdx.x * GT_PER_WG, k1 = min(nc, k0 + GT_PER_WG);
        for (int k = k0 + tid; k < k1; k += 256) {
            int x[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
            const int i = k / wc, j = k - i * wc;
            const size_t y = 2 * (size_t)i + 1, xx = 2 * (size_t)j + 1;
            x[0] = src[y * W + xx]; a[0] = src[y * W + xx - 1];
            bb[0] = src[(y - 1) * W + xx]; cc[0] = src[(y - 1) * W + xx - 1];
            gt_add4<HAS_ROI>(cnt, tid, x, a, bb, cc, pee_roi_in(R, i, j) ? 0 : 1, tmax, maxval, g_fixed);
        }
    }
    __syncthreads();
    // the workgroup's bins: thread t sums word t % nw over the lanes of group t / nw (skewed by
    // the word so that a wave's reads spread over the banks) and splits the four byte counters
    const int ngrp = 256 / nw;
    if (tid < ngrp * nw) {
        const int w = tid % nw, g = tid / nw;
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int l = g; l < 256; l += ngrp) {
            const uint32_t v = cnt[w * 256 + ((l + w) & 255)];
            s0 += v & 0xFFu; s1 += (v >> 8) & 0xFFu; s2 += (v >> 16) & 0xFFu; s3 += v >> 24;
        }
        if (s0) atomicAdd(&bins[w * 4 + 0], s0);
        if (s1) atomicAdd(&bins[w * 4 + 1], s1);
        if (s2) atomicAdd(&bins[w * 4 + 2], s2);
        if (s3) atomicAdd(&bins[w * 4 + 3], s3);
    }
    __syncthreads();
    // returning device-scope atomics, waited for: performed before the barrier and so before
    // this workgroup's arrival (no __threadfence; see k_pee_ehist)
    uint32_t* gbins = gbins_all + (size_t)b * GT_BINS;
    for (int i = tid; i < nb; i += 256)
        if (bins[i]) {
            const uint32_t prev = atomicAdd(&gbins[i], bins[i]);
            asm volatile("" ::"v"(prev));
        }
    __syncthreads();
    if (tid == 0) ticket = atomicAdd(&arrivals[b], 1u);
    __syncthreads();
    if (ticket != gridDim.x - 1u) return;
    // the slice's last workgroup: the table, then the selection
    for (int i = tid; i < nb; i += 256) bins[i] = __hip_atomic_load(gbins + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (hs_out)
        for (int i = tid; i < tmax * GT_CLASSES; i += 256) hs_out[(size_t)b * tmax * GT_CLASSES + i] = bins[i];
    if (n_out && tid < GT_CLASSES) {
        uint32_t s = 0;
        for (int r = 0; r <= tmax; ++r) s += bins[r * GT_CLASSES + tid];
        n_out[(size_t)b * GT_CLASSES + tid] = s;
    }
    if (lengths && tid == 0)
        gt_select(bins, tmax, t_fixed, g_fixed, (u64)max(0, lengths[b]), t_out ? t_out + b : nullptr,
                  g_out ? g_out + b : nullptr, k_out ? k_out + b : nullptr);
}

// the slices' global bins and arrival counters, cleared by a launch of its own before the table
// pass (a kernel node when the call is captured into a graph)
__global__ __launch_bounds__(256) void k_pee_gate_zero(uint32_t* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

static int gate_check(const codec_pee_params* P, int32_t tmax, int32_t t_fixed, int32_t g_fixed, const char* who) {
    if (!P) return set_err(CODEC_EINVAL, "%s: params is NULL", who);
    if (tmax < 1 || tmax > GT_TMAX) return set_err(CODEC_EINVAL, "%s: tmax must be in 1..16", who);
    if (t_fixed < 0 || t_fixed > tmax) return set_err(CODEC_EINVAL, "%s: t_fixed must be 0 or in 1..tmax", who);
    if (g_fixed < -1 || g_fixed > CODEC_PEE_GATE_MAX) return set_err(CODEC_EINVAL, "%s: g_fixed must be -1 or in 0..65535", who);
    if (P->H >= 1 && P->W >= 1 && (long long)(P->H / 2) * (P->W / 2) > CODEC_PEE_GATE_MAX_NC)
        return set_err(CODEC_EINVAL, "%s: more than 2^26 candidates per slice", who);
    return 0;
}

static int gate_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed, int32_t g_fixed,
                         const int32_t* lengths, const int32_t* rps, uint32_t* n, uint32_t* hs, int32_t* t_out,
                         int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes, void* stream,
                         const char* who, bool roi);

extern "C" {

size_t codec_pee_gate_workspace_bytes(const codec_pee_params* P, int32_t tmax) {
    if (gate_check(P, tmax, 0, -1, "codec_pee_gate_workspace_bytes")) return 0;
    const size_t base = codec_pee_workspace_bytes(P);   // checks P
    if (!base) return 0;
    return align_up(base, 256) + align_up((size_t)P->B * (GT_BINS + 1) * 4, 256);
}

int codec_pee_gate_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed,
                            int32_t g_fixed, const int32_t* lengths, uint32_t* n, uint32_t* hs, int32_t* t_out,
                            int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes, void* stream) {
    return gate_capacity(P, cover, tmax, t_fixed, g_fixed, lengths, nullptr, n, hs, t_out, g_out, k_out, workspace,
                         workspace_bytes, stream, "codec_pee_gate_capacity", false);
}

}  // extern "C"

// the table pass of codec_pee_gate_capacity and codec_pee_roi_capacity (rps: per-slice
// rectangles on the device, NULL for none; `roi`: the call is a ROI call and checks as one)
static int gate_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed, int32_t g_fixed,
                         const int32_t* lengths, const int32_t* rps, uint32_t* n, uint32_t* hs, int32_t* t_out,
                         int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes, void* stream,
                         const char* who, bool roi) {
    int rc = gate_check(P, tmax, t_fixed, g_fixed, who);
    if (rc) return rc;
    const size_t base = codec_pee_workspace_bytes(P);
    if (!base) return CODEC_EINVAL;   // codec_pee_workspace_bytes set the text
    if (roi && (rc = pee_roi_dim_check(P, who))) return rc;
    if (!cover || !workspace) return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    if ((t_out || g_out || k_out) && !lengths) return set_err(CODEC_EINVAL, "%s: t_out / g_out / k_out need lengths", who);
    if (workspace_bytes < codec_pee_gate_workspace_bytes(P, tmax)) return set_err(CODEC_EINVAL, "workspace too small");
    hipStream_t st = as_stream(stream);
    // the registry, as every workspace-taking call: the bins lie behind THIS shape's layout, so on
    // a workspace in use for a larger shape they fall inside that shape's state (its capacity
    // bins); recorded here, the change of shape makes the larger shape's next call zero it first
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    uint32_t* gbins = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + align_up(base, 256));
    uint32_t* arrivals = gbins + (size_t)P->B * GT_BINS;
    {
        const size_t nz = (size_t)P->B * (GT_BINS + 1);
        hipLaunchKernelGGL(k_pee_gate_zero, dim3((unsigned)std::min<size_t>(1024, (nz + 255) / 256)), dim3(256), 0, st, gbins, nz);
        LAUNCH_CHECK("k_pee_gate_zero");
    }
    const bool vec = pee_vec_route(P, cover);
    const long long units = vec ? (long long)(P->H / 2) * (P->W / 8) : (long long)(P->H / 2) * (P->W / 2);
    ProfScope prof(st, CODEC_K_PEE_GATE_TABLE);
    dim3 grid((unsigned)std::max(1LL, (units + GT_PER_WG - 1) / GT_PER_WG), (unsigned)P->B);
    auto go = [&](auto... roi) {   // roi: the rectangles, for the ROI instantiations
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            pee_flag(vec, [&](auto v) {
                hipLaunchKernelGGL((k_pee_gate_table<TT, v(), decltype(roi)...>), grid, dim3(256), 0, st,
                                   static_cast<const TT*>(cover), P->H, P->W, P->maxval, (int)tmax, (int)t_fixed, (int)g_fixed,
                                   gbins, arrivals, lengths, n, hs, t_out, g_out, k_out, roi...);
            });
        });
    };
    if (rps) go(rps); else go();
    LAUNCH_CHECK("k_pee_gate_table");
    return 0;
}

extern "C" {

int codec_pee_roi_capacity(const codec_pee_params* P, const void* cover, int32_t tmax, int32_t t_fixed,
                           int32_t g_fixed, const int32_t* lengths, const int32_t* roi, uint32_t* n, uint32_t* hs,
                           int32_t* t_out, int32_t* g_out, int32_t* k_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return gate_capacity(P, cover, tmax, t_fixed, g_fixed, lengths, roi, n, hs, t_out, g_out, k_out, workspace,
                         workspace_bytes, stream, "codec_pee_roi_capacity", true);
}

int codec_pee_roi_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                             const int32_t* lengths, int32_t tmax, int32_t t_fixed, int32_t g_fixed, const int32_t* roi,
                             int32_t* t_out, int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                             size_t workspace_bytes, void* stream) {
    int rc = gate_check(P, tmax, t_fixed, g_fixed, "codec_pee_roi_embed_auto");
    if (rc) return rc;
    if (!codec_pee_workspace_bytes(P)) return CODEC_EINVAL;   // it set the text
    if ((rc = pee_roi_dim_check(P, "codec_pee_roi_embed_auto"))) return rc;
    if (!cover || !stego || !payload || !lengths || !t_out || !g_out || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "codec_pee_roi_embed_auto: NULL pointer argument");
    rc = codec_pee_roi_capacity(P, cover, tmax, t_fixed, g_fixed, lengths, roi, nullptr, nullptr, t_out, g_out, nullptr,
                                workspace, workspace_bytes, stream);
    if (rc) return rc;
    return codec_pee_roi_embed(P, cover, stego, payload, lengths, t_out, g_out, roi, meta, lm, workspace, workspace_bytes,
                               stream);
}

int codec_pee_gate_embed_auto(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* payload,
                              const int32_t* lengths, int32_t tmax, int32_t t_fixed, int32_t g_fixed, int32_t* t_out,
                              int32_t* g_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                              size_t workspace_bytes, void* stream) {
    int rc = gate_check(P, tmax, t_fixed, g_fixed, "codec_pee_gate_embed_auto");
    if (rc) return rc;
    if (!cover || !stego || !payload || !lengths || !t_out || !g_out || !meta || !lm || !workspace)
        return set_err(CODEC_EINVAL, "codec_pee_gate_embed_auto: NULL pointer argument");
    rc = codec_pee_gate_capacity(P, cover, tmax, t_fixed, g_fixed, lengths, nullptr, nullptr, t_out, g_out, nullptr,
                                 workspace, workspace_bytes, stream);
    if (rc) return rc;
    return codec_pee_gate_embed(P, cover, stego, payload, lengths, t_out, g_out, meta, lm, workspace, workspace_bytes,
                                stream);
}

}  // extern "C"

// codec_gvol.hip -- gated MED-PEE volume payloads (include/codec_tcc_gvol.h; specification:
// tests/pee_gvol_spec.py): one bitstream planned across a slice stack over (T, G).
//
// One new kernel, k_gvol_plan, one workgroup of 1024 threads in one launch, in the style of
// codec_vol.hip's k_vol_plan<0> (no global atomics, no agent-scope fence, no "last workgroup"
// hand-off -- DESIGN §8b; static LDS only and no memset in the chain -- DESIGN §3f):
//   1. column sums over the B slices of the 16 + 16 * tmax table columns, 64-bit accumulators.
//      hs is a [B][16 tmax] matrix: thread t takes column t % 256 of the rows t / 256 + 4 k, so
//      a row is read by consecutive lanes; the four partial sums meet in LDS.  n is [B][16]: a
//      wave takes four rows at a time, the lanes of one column are reduced with shuffles and
//      the sixteen waves' partials meet in LDS.
//   2. the volume choice: 256 lanes take one (T, j) pair each from the summed table, then a
//      shuffle / LDS reduction under the rule's total order, A1 K2 < A2 K1 compared as 128-bit
//      products (__umul64hi + the plain product), ties by T, then j.
//   3. rounds of 1024 slices: c_b = K_b(T*, j*) from slice b's table (at most 256 adds), the
//      block-wide 64-bit exclusive scan with a carry (block_excl_scan64, as k_vol_plan), n_b
//      and off_b in closed form from P_b, then the per-slice selection gv_select, one thread
//      per slice, on the slice's own table with L = n_b (32-bit sums, 64-bit products).
// The per-slice selection walks j outward and T inward so that it needs sixteen running sums (the rows'
// sums over the classes <= j) where k_pee_gate_table's gt_select, walking T outward, keeps
// three per class; the tie-break is explicit (smaller T, then smaller j) and the tests pin the
// two to the same answers.  Table values are clamped to (H/2)(W/2) as they are read.
// The decode side needs no kernel of its own: k_vol_plan<1> scans the records' L.
#include "codec_vol_checks.h"
#include "codec_tcc_gvol.h"

#define GV_NT 1024
#define GV_CLASSES CODEC_PEE_GATE_CLASSES
#define GV_TMAX CODEC_PEE_GATE_TMAX

// a1 * k2 < a2 * k1 as 128-bit products, exactly; *eq: the products are equal
__device__ __forceinline__ bool gv_less128(u64 a1, u64 k1, u64 a2, u64 k2, bool* eq) {
    const u64 l1 = a1 * k2, l2 = a2 * k1;
    const u64 h1 = __umul64hi(a1, k2), h2 = __umul64hi(a2, k1);
    *eq = (h1 == h2) & (l1 == l2);
    return h1 < h2 || (h1 == h2 && l1 < l2);
}

// A candidate pair of the volume choice is (A, K, idx, ok): idx = (T - 1) * 16 + j orders the
// ties (smaller T, then smaller j), ok = feasible.
// (A, K, idx, ok) becomes the better of itself and (A2, K2, idx2, ok2)
__device__ __forceinline__ void gv_merge(u64& A, u64& K, int& idx, int& ok, u64 A2, u64 K2, int idx2, int ok2) {
    bool eq;
    const bool lt = gv_less128(A2, K2, A, K, &eq);
    const bool take = ok2 && (!ok || lt || (eq && idx2 < idx));
    A = take ? A2 : A;
    K = take ? K2 : K;
    idx = take ? idx2 : idx;
    ok = take ? ok2 : ok;
}

// The selection rule of include/codec_tcc_gate.h on one slice's table, read through hs(u, j) and
// n(j) (uint32: a slice's sums stay below 2^27, so K, N and the row sums are 32-bit, A and the
// cost sum below 2^36 and every product one 64 x 32 multiply).  g_fixed >= 0: the smallest T
// whose K(T, 0) holds L.  *t_out in 1..tmax, *j_out in 0..15 (0 for a fixed gate).
template <typename HS, typename NN>
__device__ __forceinline__ void gv_select(HS hs, NN n, int tmax, int g_fixed, uint32_t L, int* t_out, int* j_out) {
    if (g_fixed >= 0) {
        uint32_t K = 0;
        int T = 1;
        for (; T <= tmax; ++T) {
            K += hs(T - 1, 0);
            if (K >= L) break;
        }
        *t_out = min(T, tmax);
        *j_out = 0;
        return;
    }
    uint32_t rs[GV_TMAX];   // rs[u] = sum of hs[u][g] over g <= j
#pragma unroll
    for (int u = 0; u < GV_TMAX; ++u) rs[u] = 0u;
    bool have = false;
    u64 bestA = 0;
    uint32_t bestK = 0, N = 0;
    int bestT = tmax, bestJ = GV_CLASSES - 1;
    for (int j = 0; j < GV_CLASSES; ++j) {
        N += n(j);
        uint32_t K = 0;
        u64 S = 0;
        // the row's cost u^2 + (u + 1)^2 and 2 T^2 as running values the compiler cannot fold:
        // as constants of the unrolled loop they are some fifty scalar registers that live
        // across the whole walk and spill
        uint32_t cost = 1u, tt2 = 2u;
        asm volatile("" : "+v"(cost), "+v"(tt2));
#pragma unroll
        for (int u = 0; u < GV_TMAX; ++u) {
            if (u < tmax) {
                const int T = u + 1;
                rs[u] += hs(u, j);
                K += rs[u];
                S += (u64)rs[u] * cost;
                const u64 A = (u64)tt2 * (uint32_t)(N - K) + S;
                if (L == 0) {   // nothing to embed: the first pair visited, (1, 0)
                    if (!have) { have = true; bestA = A; bestK = K; bestT = T; bestJ = j; }
                } else if (K >= L) {
                    const u64 l1 = A * (u64)bestK, l2 = bestA * (u64)K;   // below 2^63
                    if (!have || l1 < l2 || (l1 == l2 && T < bestT)) { have = true; bestA = A; bestK = K; bestT = T; bestJ = j; }
                }
                cost += 4u * u + 4u;
                tt2 += 4u * u + 6u;
            }
        }
    }
    *t_out = bestT;
    *j_out = bestJ;
}

__global__ __launch_bounds__(GV_NT) void k_gvol_plan(const uint32_t* __restrict__ ntab, const uint32_t* __restrict__ hstab,
                                                    int B, int tmax, uint32_t capmax, u64 nbits, int policy,
                                                    int g_fixed, int32_t* __restrict__ n_out,
                                                    int32_t* __restrict__ t_out, int32_t* __restrict__ g_out,
                                                    int32_t* __restrict__ off_out,
                                                    codec_pee_gvol_info* __restrict__ info) {
    __shared__ u64 s_scan[GV_NT / 64 + 1];
    __shared__ u64 s_hp[4][GV_TMAX * GV_CLASSES];   // hs: partial sums of the four row groups
    __shared__ u64 s_np[GV_NT / 64][GV_CLASSES];    // n: partial sums of the sixteen waves
    __shared__ u64 s_hs[GV_TMAX * GV_CLASSES];
    __shared__ u64 s_n[GV_CLASSES];
    __shared__ u64 s_N, s_kmax;
    __shared__ u64 s_cA[4], s_cK[4];   // the four waves' best pairs
    __shared__ int s_ci[4], s_co[4];
    __shared__ int s_t, s_j, s_status;
    const int gates[GV_CLASSES] = {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535};
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ncol = tmax * GV_CLASSES;
    {
        const int col = tid & 255, grp = tid >> 8;
        u64 acc = 0;
        if (col < ncol)
            for (int r = grp; r < B; r += 4) acc += (u64)min(hstab[(size_t)r * ncol + col], capmax);
        s_hp[grp][col] = acc;
        const int c = lane & 15, sub = lane >> 4;
        u64 an = 0;
        for (int r = wv * 4 + sub; r < B; r += (GV_NT / 64) * 4) an += (u64)min(ntab[(size_t)r * GV_CLASSES + c], capmax);
        an += __shfl_xor(an, 32, 64);
        an += __shfl_xor(an, 16, 64);
        if (lane < GV_CLASSES) s_np[wv][lane] = an;
    }
    __syncthreads();
    if (tid < ncol) s_hs[tid] = s_hp[0][tid] + s_hp[1][tid] + s_hp[2][tid] + s_hp[3][tid];
    if (tid >= 256 && tid < 256 + GV_CLASSES) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < GV_NT / 64; ++w) s += s_np[w][tid - 256];
        s_n[tid - 256] = s;
    }
    __syncthreads();
    // the volume choice: thread (T - 1) * 16 + j rates its pair from the summed table, then a
    // reduction under the rule's total order (A / K by 128-bit cross-products, then T, then j)
    if (g_fixed >= 0) {
        if (tid == 0) {   // one column: the smallest T that holds N
            u64 K = 0;
            int T = 1;
            for (; T <= tmax; ++T) {
                K += s_hs[(T - 1) * GV_CLASSES];
                if (K >= nbits) break;
            }
            s_status = T > tmax;
            s_t = min(T, tmax);
            s_j = 0;
            s_N = T > tmax ? K : nbits;
        }
    } else if (tid < GV_TMAX * GV_CLASSES) {   // waves 0..3, whole
        const int T = tid / GV_CLASSES + 1, j = tid % GV_CLASSES;
        u64 cA = 0, cK = 0;
        int ci = tid, co = 0;
        if (T <= tmax) {
            u64 K = 0, S = 0, Nj = 0;
            for (int g = 0; g <= j; ++g) Nj += s_n[g];
            for (int u = 0; u < T; ++u) {
                u64 r = 0;
                for (int g = 0; g <= j; ++g) r += s_hs[u * GV_CLASSES + g];
                K += r;
                S += r * (u64)(u * u + (u + 1) * (u + 1));
            }
            cA = 2ull * (u64)(T * T) * (Nj - K) + S;
            cK = K;
            co = nbits == 0 ? tid == 0 : K >= nbits;   // N = 0: (1, 0)
            if (T == tmax && j == GV_CLASSES - 1) s_kmax = K;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const u64 dA = __shfl_xor(cA, o, 64), dK = __shfl_xor(cK, o, 64);
            const int di = __shfl_xor(ci, o, 64), dn = __shfl_xor(co, o, 64);
            gv_merge(cA, cK, ci, co, dA, dK, di, dn);
        }
        if (lane == 0) { s_cA[wv] = cA; s_cK[wv] = cK; s_ci[wv] = ci; s_co[wv] = co; }
    }
    __syncthreads();
    if (g_fixed < 0 && tid == 0) {
        u64 cA = s_cA[0], cK = s_cK[0];
        int ci = s_ci[0], co = s_co[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) gv_merge(cA, cK, ci, co, s_cA[w], s_cK[w], s_ci[w], s_co[w]);
        s_status = !co;
        s_t = co ? ci / GV_CLASSES + 1 : tmax;
        s_j = co ? ci % GV_CLASSES : GV_CLASSES - 1;
        s_N = co ? nbits : s_kmax;
    }
    __syncthreads();
    const int T = s_t, J = s_j;
    const u64 N = s_N;
    // P_B: the clamped shares' sum, known only after the scan -- a first pass over the slices
    u64 carry = 0;
    for (int base = 0; base < B; base += GV_NT) {
        const int b = base + tid;
        u64 c = 0;
        if (b < B) {
            const uint32_t* h = hstab + (size_t)b * ncol;
            for (int u = 0; u < T; ++u)
                for (int g = 0; g <= J; ++g) c += (u64)min(h[u * GV_CLASSES + g], capmax);
            c = min(c, (u64)capmax);
        }
        u64 tot;
        (void)block_excl_scan64<GV_NT>(c, s_scan, &tot);
        carry += tot;
        if (B - base <= GV_NT) break;   // (base + GV_NT could pass INT_MAX)
    }
    const u64 PB = carry;
    // a truncated stream is cut to what the clamped shares hold (equal to N on real tables)
    const u64 NN = min(N, PB);
    carry = 0;
    for (int base = 0; base < B; base += GV_NT) {
        const int b = base + tid;
        const uint32_t* h = hstab + (size_t)(b < B ? b : 0) * ncol;
        const uint32_t* nn = ntab + (size_t)(b < B ? b : 0) * GV_CLASSES;
        u64 c = 0;
        if (b < B) {
            for (int u = 0; u < T; ++u)
                for (int g = 0; g <= J; ++g) c += (u64)min(h[u * GV_CLASSES + g], capmax);
            c = min(c, (u64)capmax);
        }
        u64 tot;
        const u64 Pb = carry + block_excl_scan64<GV_NT>(c, s_scan, &tot);
        carry += tot;
        if (b < B) {
            u64 off, n;
            if (policy == CODEC_VOL_FILL) {
                off = min(NN, Pb);
                n = min(c, NN - off);
            } else {
                off = PB ? NN * Pb / PB : 0ull;   // N, P < 2^31: the products stay below 2^62
                n = (PB ? NN * (Pb + c) / PB : 0ull) - off;
            }
            int tb, jb;
            gv_select([&](int u, int jj) { return min(h[u * GV_CLASSES + jj], capmax); },
                      [&](int jj) { return min(nn[jj], capmax); }, tmax, g_fixed, (uint32_t)n, &tb, &jb);
            n_out[b] = (int32_t)n;
            t_out[b] = tb;
            g_out[b] = g_fixed >= 0 ? g_fixed : gates[jb];
            off_out[b] = (int32_t)off;
        }
        if (B - base <= GV_NT) break;
    }
    if (tid == 0) {
        off_out[B] = (int32_t)NN;
        info->status = s_status;
        info->T = T;
        info->total = (int32_t)NN;
        info->requested = (int32_t)nbits;
        info->capacity = (int32_t)PB;
        info->policy = policy;
        info->B = B;
        info->tmax = tmax;
        info->gate = g_fixed >= 0 ? g_fixed : gates[J];
        info->reserved = 0;
    }
}

// ====================================================================== host side
// the checks are codec_vol_checks.h's, with the gate's bound on a slice's candidates
static int gvol_check(const codec_pee_params* P, const char* who) { return vol_check(P, who, CODEC_PEE_GATE_MAX_NC); }

// the workspace: the volume head (codec_pee_volume_gather takes this workspace as it is), then
// the tables n [B][16] and hs [B][tmax][16]
struct GvolWs : VolWsHead {
    size_t ntab, hstab, total;
};
static GvolWs gvol_ws(const codec_pee_params* P, int32_t tmax) {
    GvolWs L;
    static_cast<VolWsHead&>(L) = vol_ws_head(P);
    L.ntab = L.end;
    L.hstab = align_up(L.ntab + (size_t)P->B * GV_CLASSES * 4, 256);
    L.total = align_up(L.hstab + (size_t)P->B * tmax * GV_CLASSES * 4, 256);
    return L;
}

static int gvol_launch_plan(const codec_pee_params* P, const uint32_t* n, const uint32_t* hs, int32_t tmax,
                            int64_t nbits, int32_t policy, int32_t g_fixed, int32_t* n_out, int32_t* t_out,
                            int32_t* g_out, int32_t* off_out, codec_pee_gvol_info* info, hipStream_t st) {
    ProfScope prof(st, CODEC_K_GVOL_PLAN);
    hipLaunchKernelGGL(k_gvol_plan, dim3(1), dim3(GV_NT), 0, st, n, hs, (int)P->B, (int)tmax, (uint32_t)vol_nc(P),
                       (u64)nbits, (int)policy, (int)g_fixed, n_out, t_out, g_out, off_out, info);
    LAUNCH_CHECK("k_gvol_plan");
    return 0;
}

extern "C" {

size_t codec_pee_gvol_workspace_bytes(const codec_pee_params* P, int32_t tmax) {
    if (gvol_check(P, "codec_pee_gvol_workspace_bytes")) return 0;
    if (vol_check_tmax(tmax, GV_TMAX, "codec_pee_gvol_workspace_bytes")) return 0;
    return gvol_ws(P, tmax).total;
}

int codec_pee_gvol_plan(const codec_pee_params* P, const uint32_t* n, const uint32_t* hs, int32_t tmax, int64_t nbits,
                        int32_t policy, int32_t g_fixed, int32_t* n_out, int32_t* t_out, int32_t* g_out,
                        int32_t* off_out, codec_pee_gvol_info* info, void* stream) {
    int rc = gvol_check(P, "codec_pee_gvol_plan");
    if (rc) return rc;
    if ((rc = vol_check_plan(P, tmax, GV_TMAX, nbits, policy, g_fixed, "codec_pee_gvol_plan"))) return rc;
    if (!n || !hs || !n_out || !t_out || !g_out || !off_out || !info)
        return set_err(CODEC_EINVAL, "codec_pee_gvol_plan: NULL pointer argument");
    return gvol_launch_plan(P, n, hs, tmax, nbits, policy, g_fixed, n_out, t_out, g_out, off_out, info,
                            as_stream(stream));
}

int codec_pee_gvol_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                         int64_t nbits, int32_t policy, int32_t tmax, int32_t g_fixed, int32_t* n_out, int32_t* t_out,
                         int32_t* g_out, int32_t* off_out, codec_pee_gvol_info* info, codec_pee_meta* meta,
                         uint64_t* lm, void* pee_workspace, size_t pee_workspace_bytes, void* table_workspace,
                         size_t table_workspace_bytes, void* gvol_workspace, size_t gvol_workspace_bytes, void* stream) {
    int rc = gvol_check(P, "codec_pee_gvol_embed");
    if (rc) return rc;
    if ((rc = vol_check_plan(P, tmax, GV_TMAX, nbits, policy, g_fixed, "codec_pee_gvol_embed"))) return rc;
    if (!cover || !stego || !n_out || !t_out || !g_out || !off_out || !info || !meta || !lm || !pee_workspace ||
        !table_workspace || !gvol_workspace || (!bitstream && nbits > 0))
        return set_err(CODEC_EINVAL, "codec_pee_gvol_embed: NULL pointer argument");
    if ((rc = vol_check_pee_ws(P, pee_workspace_bytes, "codec_pee_gvol_embed"))) return rc;
    const size_t need_tab = codec_pee_gate_workspace_bytes(P, tmax);
    if (!need_tab || table_workspace_bytes < need_tab)
        return set_err(CODEC_EINVAL, "codec_pee_gvol_embed: table workspace too small (%zu < %zu)",
                       table_workspace_bytes, need_tab);
    const GvolWs L = gvol_ws(P, tmax);
    if (gvol_workspace_bytes < L.total)
        return set_err(CODEC_EINVAL, "codec_pee_gvol_embed: gated volume workspace too small (%zu < %zu)",
                       gvol_workspace_bytes, L.total);
    char* w = static_cast<char*>(gvol_workspace);
    uint32_t* ntab = reinterpret_cast<uint32_t*>(w + L.ntab);
    uint32_t* hstab = reinterpret_cast<uint32_t*>(w + L.hstab);
    uint64_t* rows = reinterpret_cast<uint64_t*>(w + L.rows);
    if ((rc = codec_pee_gate_capacity(P, cover, tmax, 0, g_fixed, nullptr, ntab, hstab, nullptr, nullptr, nullptr,
                                      table_workspace, table_workspace_bytes, stream)))
        return rc;
    if ((rc = gvol_launch_plan(P, ntab, hstab, tmax, nbits, policy, g_fixed, n_out, t_out, g_out, off_out, info,
                               as_stream(stream))))
        return rc;
    if ((rc = codec_pee_volume_scatter(P, bitstream, nbits, n_out, off_out, rows, stream))) return rc;
    return codec_pee_gate_embed(P, cover, stego, rows, n_out, t_out, g_out, meta, lm, pee_workspace,
                                pee_workspace_bytes, stream);
}

int codec_pee_gvol_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta, const uint64_t* lm,
                           void* cover_out, uint64_t* bitstream, int64_t stream_words, int32_t* total_out,
                           void* pee_workspace, size_t pee_workspace_bytes, void* gvol_workspace,
                           size_t gvol_workspace_bytes, void* stream) {
    int rc = gvol_check(P, "codec_pee_gvol_extract");
    if (rc) return rc;
    if ((rc = vol_check_stream_words(stream_words, "codec_pee_gvol_extract"))) return rc;
    if (!stego || !meta || !lm || !cover_out || !total_out || !pee_workspace || !gvol_workspace ||
        (!bitstream && stream_words > 0))
        return set_err(CODEC_EINVAL, "codec_pee_gvol_extract: NULL pointer argument");
    if ((rc = vol_check_pee_ws(P, pee_workspace_bytes, "codec_pee_gvol_extract"))) return rc;
    const GvolWs L = gvol_ws(P, 1);
    if (gvol_workspace_bytes < L.total)
        return set_err(CODEC_EINVAL, "codec_pee_gvol_extract: gated volume workspace too small (%zu < %zu)",
                       gvol_workspace_bytes, L.total);
    uint64_t* rows = reinterpret_cast<uint64_t*>(static_cast<char*>(gvol_workspace) + L.rows);
    if ((rc = codec_pee_gate_extract(P, stego, meta, lm, cover_out, rows, pee_workspace, pee_workspace_bytes, stream)))
        return rc;
    return codec_pee_volume_gather(P, meta, rows, bitstream, stream_words, total_out, gvol_workspace,
                                   gvol_workspace_bytes, stream);
}

}  // extern "C"

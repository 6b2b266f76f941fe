// codec_vol.hip -- MED-PEE volume payloads (include/codec_tcc_vol.h): one bitstream planned
// across a slice stack, cut into the per-slice payload rows codec_pee_embed_ts takes, and put
// together again from the rows codec_pee_extract returns.
//
// Three kernels, three launches; a kernel boundary is the ordering between them (no "last
// workgroup" hand-off: DESIGN §8b prices an agent-scope release on this part).
//   k_vol_plan<0>  one workgroup of 1024 threads: column sums of caps per T (wave reductions,
//                  then LDS), T* and the status, then a block-wide exclusive scan of the slices'
//                  capacities at T* in rounds of 1024 with a carry.  P_b gives n_b and off_b in
//                  closed form for both policies (even: off_b = floor(N P_b / P_B); fill:
//                  off_b = min(N, P_b)), so one scan serves n, T and off.  No atomics.
//   k_vol_plan<1>  the decode side's offsets: the same scan over the records' L.
//   k_vol_scatter  one thread per row word: a funnel shift of two stream words, masked at the
//                  row's last partial word, zero above n_b.
//   k_vol_gather   one thread per stream word: a binary search in off for the first slice that
//                  contributes, then a walk over slices (runs of empty ones included) until the
//                  word's 64 bits are filled.  Each word is written once.
#include "codec_vol_checks.h"

#define VOL_NT 1024
#define VOL_TMAX 64

__device__ __forceinline__ u64 vol_clamp(int32_t v, uint32_t hi) {
    return (u64)min((uint32_t)max(v, 0), hi);
}

// exclusive prefix of x over the threads of this round plus the rounds before it
__device__ __forceinline__ u64 vol_scan_round(u64 x, u64* sh, u64& carry) {
    u64 tot;
    const u64 ex = block_excl_scan64<VOL_NT>(x, sh, &tot);
    const u64 r = carry + ex;
    carry += tot;
    return r;
}

// MODE 0: the plan.  MODE 1: off[b] = exclusive prefix of the records' bounded L, off[B] and
// *total_out = their sum (caps, tmax, nbits, policy, n_out, t_out, info unused).
template <int MODE>
__global__ __launch_bounds__(VOL_NT) void k_vol_plan(const int32_t* __restrict__ caps,
                                                     const codec_pee_meta* __restrict__ meta, int B, int tmax,
                                                     uint32_t capmax, u64 nbits, int policy,
                                                     int32_t* __restrict__ n_out, int32_t* __restrict__ t_out,
                                                     int32_t* __restrict__ off_out,
                                                     codec_pee_volume_info* __restrict__ info,
                                                     int32_t* __restrict__ total_out) {
    __shared__ u64 s_scan[VOL_NT / 64 + 1];
    const int tid = threadIdx.x;
    u64 carry = 0;
    if constexpr (MODE == 1) {
        for (int base = 0; base < B; base += VOL_NT) {
            const int b = base + tid;
            const u64 x = b < B ? vol_clamp(meta[b].L, capmax) : 0ull;
            const u64 pre = vol_scan_round(x, s_scan, carry);
            if (b < B) off_out[b] = (int32_t)pre;
            if (B - base <= VOL_NT) break;   // (base + VOL_NT could pass INT_MAX)
        }
        if (tid == 0) {
            off_out[B] = (int32_t)carry;
            *total_out = (int32_t)carry;
        }
        return;
    } else {
        __shared__ u64 s_part[VOL_NT / 64][VOL_TMAX];
        __shared__ u64 s_sum[VOL_TMAX];
        __shared__ u64 s_n;
        __shared__ int s_t, s_status;
        const int lane = tid & 63, wv = tid >> 6;
        // lanes of one wave: tp columns (the power of two >= tmax) by 64 / tp rows
        int tp = 1;
        while (tp < tmax) tp <<= 1;
        const int col = lane & (tp - 1), sub = lane / tp, rpw = 64 / tp;
        u64 acc = 0;
        if (col < tmax)
            for (long long r = (long long)wv * rpw + sub; r < B; r += (long long)(VOL_NT / 64) * rpw)
                acc += vol_clamp(caps[(size_t)r * tmax + col], capmax);
        for (int o = 32; o >= tp; o >>= 1) acc += __shfl_xor(acc, o, 64);   // the lanes of one column
        if (lane < tp) s_part[wv][lane] = acc;
        __syncthreads();
        if (tid < tmax) {
            u64 s = 0;
#pragma unroll
            for (int w = 0; w < VOL_NT / 64; ++w) s += s_part[w][tid];
            s_sum[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 1;
            while (t <= tmax && s_sum[t - 1] < nbits) ++t;
            const int st = t > tmax;
            s_t = st ? tmax : t;
            s_status = st;
            s_n = st ? s_sum[tmax - 1] : nbits;
        }
        __syncthreads();
        const int T = s_t;
        const u64 N = s_n, PB = s_sum[T - 1];
        for (int base = 0; base < B; base += VOL_NT) {
            const int b = base + tid;
            const int32_t* row = caps + (size_t)(b < B ? b : 0) * tmax;
            const u64 c = b < B ? vol_clamp(row[T - 1], capmax) : 0ull;
            const u64 Pb = vol_scan_round(c, s_scan, carry);
            if (b < B) {
                u64 off, n;
                if (policy == CODEC_VOL_FILL) {
                    off = min(N, Pb);
                    n = min(c, N - off);
                } else {
                    off = PB ? N * Pb / PB : 0ull;   // N, P < 2^31: the products stay below 2^62
                    n = (PB ? N * (Pb + c) / PB : 0ull) - off;
                }
                int t = 1;
                while (t < T && vol_clamp(row[t - 1], capmax) < n) ++t;   // caps[b][T-1] = c >= n
                n_out[b] = (int32_t)n;
                t_out[b] = t;
                off_out[b] = (int32_t)off;
            }
            if (B - base <= VOL_NT) break;
        }
        if (tid == 0) {
            off_out[B] = (int32_t)N;
            info->status = s_status;
            info->T = T;
            info->total = (int32_t)N;
            info->requested = (int32_t)nbits;
            info->capacity = (int32_t)PB;
            info->policy = policy;
            info->B = B;
            info->tmax = tmax;
        }
    }
}

__global__ __launch_bounds__(256) void k_vol_scatter(const u64* __restrict__ bits, u64 stream_words,
                                                     const int32_t* __restrict__ n, const int32_t* __restrict__ off,
                                                     uint32_t nwords, uint32_t pw, u64* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t b = i / pw, w = i - b * pw;
    const long long nb = min((long long)max(n[b], 0), 64ll * pw);
    u64 v = 0;
    if (64ll * w < nb) {
        const long long p = (long long)max(off[b], 0) + 64ll * w;
        const u64 idx = (u64)p >> 6;
        const int sh = (int)(p & 63);
        const long long rem = min(nb - 64ll * w, 64ll);
        v = (idx < stream_words ? bits[idx] : 0ull) >> sh;
        if (sh && 64 - sh < rem) v |= (idx + 1 < stream_words ? bits[idx + 1] : 0ull) << (64 - sh);
        if (rem < 64) v &= (1ull << rem) - 1ull;
    }
    rows[i] = v;
}

__global__ __launch_bounds__(256) void k_vol_gather(const u64* __restrict__ rows, const int32_t* __restrict__ off,
                                                    int B, uint32_t pw, u64* __restrict__ bits, u64 stream_words) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= stream_words) return;
    const long long total = off[B];
    long long pos = (long long)(j << 6);
    u64 v = 0;
    if (pos < total) {
        int lo = 0, hi = B;   // the last slice with off[b] <= pos: it holds bit pos (off[b + 1] > pos)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= pos) lo = mid; else hi = mid;
        }
        int filled = 0;
        long long ob = off[lo];
        for (int b = lo; b < B && filled < 64; ++b) {
            const long long oe = off[b + 1];
            if (oe > pos) {
                const long long r = pos - ob;
                const int cnt = (int)min(oe - pos, (long long)(64 - filled));
                const uint32_t wi = (uint32_t)(r >> 6);
                const int sh = (int)(r & 63);
                const u64* row = rows + (size_t)b * pw;
                u64 x = (wi < pw ? row[wi] : 0ull) >> sh;
                if (sh && 64 - sh < cnt) x |= (wi + 1 < pw ? row[wi + 1] : 0ull) << (64 - sh);
                if (cnt < 64) x &= (1ull << cnt) - 1ull;
                v |= x << filled;
                filled += cnt;
                pos += cnt;
            }
            ob = oe;
        }
    }
    bits[j] = v;
}

// ====================================================================== host side
// the checks are codec_vol_checks.h's; the workspace: its head, then the capacities [B][tmax]
struct VolWs : VolWsHead {
    size_t caps, total;
};
static VolWs vol_ws(const codec_pee_params* P, int32_t tmax) {
    VolWs L;
    static_cast<VolWsHead&>(L) = vol_ws_head(P);
    L.caps = L.end;
    L.total = align_up(L.caps + (size_t)P->B * tmax * 4, 256);
    return L;
}

static uint32_t vol_capmax(const codec_pee_params* P) {
    return (uint32_t)std::min<long long>(64ll * P->payload_words, vol_nc(P));
}

static int vol_launch_plan(const codec_pee_params* P, const int32_t* caps, int32_t tmax, int64_t nbits, int32_t policy,
                           int32_t* n_out, int32_t* t_out, int32_t* off_out, codec_pee_volume_info* info,
                           hipStream_t st) {
    ProfScope prof(st, CODEC_K_VOL_PLAN);
    hipLaunchKernelGGL(k_vol_plan<0>, dim3(1), dim3(VOL_NT), 0, st, caps, (const codec_pee_meta*)nullptr, (int)P->B,
                       (int)tmax, (uint32_t)vol_nc(P), (u64)nbits, (int)policy, n_out, t_out, off_out, info,
                       (int32_t*)nullptr);
    LAUNCH_CHECK("k_vol_plan");
    return 0;
}

static int vol_launch_scatter(const codec_pee_params* P, const uint64_t* bitstream, int64_t nbits, const int32_t* n,
                              const int32_t* off, uint64_t* rows, hipStream_t st) {
    const uint32_t nwords = (uint32_t)((long long)P->B * P->payload_words);
    ProfScope prof(st, CODEC_K_VOL_SCATTER);
    hipLaunchKernelGGL(k_vol_scatter, dim3((nwords + 255u) / 256u), dim3(256), 0, st,
                       reinterpret_cast<const u64*>(bitstream), (u64)((nbits + 63) / 64), n, off, nwords,
                       (uint32_t)P->payload_words, reinterpret_cast<u64*>(rows));
    LAUNCH_CHECK("k_vol_scatter");
    return 0;
}

static int vol_launch_gather(const codec_pee_params* P, const codec_pee_meta* meta, const uint64_t* rows,
                             uint64_t* bitstream, int64_t stream_words, int32_t* total_out, int32_t* off,
                             hipStream_t st) {
    {
        ProfScope prof(st, CODEC_K_VOL_PLAN);
        hipLaunchKernelGGL(k_vol_plan<1>, dim3(1), dim3(VOL_NT), 0, st, (const int32_t*)nullptr, meta, (int)P->B, 0,
                           vol_capmax(P), 0ull, 0, (int32_t*)nullptr, (int32_t*)nullptr, off,
                           (codec_pee_volume_info*)nullptr, total_out);
        LAUNCH_CHECK("k_vol_plan");
    }
    if (stream_words > 0) {
        ProfScope prof(st, CODEC_K_VOL_GATHER);
        hipLaunchKernelGGL(k_vol_gather, dim3((unsigned)((stream_words + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const u64*>(rows), off, (int)P->B, (uint32_t)P->payload_words,
                           reinterpret_cast<u64*>(bitstream), (u64)stream_words);
        LAUNCH_CHECK("k_vol_gather");
    }
    return 0;
}

extern "C" {

size_t codec_pee_volume_workspace_bytes(const codec_pee_params* P, int32_t tmax) {
    if (vol_check(P, "codec_pee_volume_workspace_bytes")) return 0;
    if (vol_check_tmax(tmax, VOL_TMAX, "codec_pee_volume_workspace_bytes")) return 0;
    return vol_ws(P, tmax).total;
}

int codec_pee_volume_plan(const codec_pee_params* P, const int32_t* caps, int32_t tmax, int64_t nbits, int32_t policy,
                          int32_t* n_out, int32_t* t_out, int32_t* off_out, codec_pee_volume_info* info,
                          void* stream) {
    int rc = vol_check(P, "codec_pee_volume_plan");
    if (rc) return rc;
    if ((rc = vol_check_plan(P, tmax, VOL_TMAX, nbits, policy, -1, "codec_pee_volume_plan"))) return rc;
    if (!caps || !n_out || !t_out || !off_out || !info)
        return set_err(CODEC_EINVAL, "codec_pee_volume_plan: NULL pointer argument");
    return vol_launch_plan(P, caps, tmax, nbits, policy, n_out, t_out, off_out, info, as_stream(stream));
}

int codec_pee_volume_scatter(const codec_pee_params* P, const uint64_t* bitstream, int64_t nbits, const int32_t* n,
                             const int32_t* off, uint64_t* rows, void* stream) {
    int rc = vol_check(P, "codec_pee_volume_scatter");
    if (rc) return rc;
    if (nbits < 0 || nbits > 0x7FFFFFFFLL)
        return set_err(CODEC_EINVAL, "codec_pee_volume_scatter: nbits must be in 0..2^31 - 1");
    if (!n || !off || !rows || (!bitstream && nbits > 0))
        return set_err(CODEC_EINVAL, "codec_pee_volume_scatter: NULL pointer argument");
    return vol_launch_scatter(P, bitstream, nbits, n, off, rows, as_stream(stream));
}

int codec_pee_volume_gather(const codec_pee_params* P, const codec_pee_meta* meta, const uint64_t* rows,
                            uint64_t* bitstream, int64_t stream_words, int32_t* total_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    int rc = vol_check(P, "codec_pee_volume_gather");
    if (rc) return rc;
    if ((rc = vol_check_stream_words(stream_words, "codec_pee_volume_gather"))) return rc;
    if (!meta || !rows || !total_out || !workspace || (!bitstream && stream_words > 0))
        return set_err(CODEC_EINVAL, "codec_pee_volume_gather: NULL pointer argument");
    const VolWs L = vol_ws(P, 1);
    if (workspace_bytes < L.total)
        return set_err(CODEC_EINVAL, "codec_pee_volume_gather: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    int32_t* off = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.off);
    return vol_launch_gather(P, meta, rows, bitstream, stream_words, total_out, off, as_stream(stream));
}

int codec_pee_volume_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                           int64_t nbits, int32_t policy, int32_t tmax, int32_t* n_out, int32_t* t_out,
                           int32_t* off_out, codec_pee_volume_info* info, codec_pee_meta* meta, uint64_t* lm,
                           void* pee_workspace, size_t pee_workspace_bytes, void* vol_workspace,
                           size_t vol_workspace_bytes, void* stream) {
    int rc = vol_check(P, "codec_pee_volume_embed");
    if (rc) return rc;
    if ((rc = vol_check_plan(P, tmax, VOL_TMAX, nbits, policy, -1, "codec_pee_volume_embed"))) return rc;
    if (!cover || !stego || !n_out || !t_out || !off_out || !info || !meta || !lm || !pee_workspace || !vol_workspace ||
        (!bitstream && nbits > 0))
        return set_err(CODEC_EINVAL, "codec_pee_volume_embed: NULL pointer argument");
    if ((rc = vol_check_pee_ws(P, pee_workspace_bytes, "codec_pee_volume_embed"))) return rc;
    const VolWs L = vol_ws(P, tmax);
    if (vol_workspace_bytes < L.total)
        return set_err(CODEC_EINVAL, "codec_pee_volume_embed: volume workspace too small (%zu < %zu)",
                       vol_workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char* w = static_cast<char*>(vol_workspace);
    int32_t* caps = reinterpret_cast<int32_t*>(w + L.caps);
    uint64_t* rows = reinterpret_cast<uint64_t*>(w + L.rows);
    if ((rc = codec_pee_capacity(P, cover, tmax, nullptr, caps, nullptr, pee_workspace, pee_workspace_bytes, stream)))
        return rc;
    if ((rc = vol_launch_plan(P, caps, tmax, nbits, policy, n_out, t_out, off_out, info, st))) return rc;
    if ((rc = vol_launch_scatter(P, bitstream, nbits, n_out, off_out, rows, st))) return rc;
    return codec_pee_embed_ts(P, cover, stego, rows, n_out, t_out, meta, lm, pee_workspace, pee_workspace_bytes, stream);
}

int codec_pee_volume_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta,
                             const uint64_t* lm, void* cover_out, uint64_t* bitstream, int64_t stream_words,
                             int32_t* total_out, void* pee_workspace, size_t pee_workspace_bytes, void* vol_workspace,
                             size_t vol_workspace_bytes, void* stream) {
    int rc = vol_check(P, "codec_pee_volume_extract");
    if (rc) return rc;
    if ((rc = vol_check_stream_words(stream_words, "codec_pee_volume_extract"))) return rc;
    if (!stego || !meta || !lm || !cover_out || !total_out || !pee_workspace || !vol_workspace ||
        (!bitstream && stream_words > 0))
        return set_err(CODEC_EINVAL, "codec_pee_volume_extract: NULL pointer argument");
    if ((rc = vol_check_pee_ws(P, pee_workspace_bytes, "codec_pee_volume_extract"))) return rc;
    const VolWs L = vol_ws(P, 1);
    if (vol_workspace_bytes < L.total)
        return set_err(CODEC_EINVAL, "codec_pee_volume_extract: volume workspace too small (%zu < %zu)",
                       vol_workspace_bytes, L.total);
    char* w = static_cast<char*>(vol_workspace);
    uint64_t* rows = reinterpret_cast<uint64_t*>(w + L.rows);
    if ((rc = codec_pee_extract(P, stego, meta, lm, cover_out, rows, pee_workspace, pee_workspace_bytes, stream)))
        return rc;
    return vol_launch_gather(P, meta, rows, bitstream, stream_words, total_out,
                             reinterpret_cast<int32_t*>(w + L.off), as_stream(stream));
}

}  // extern "C"

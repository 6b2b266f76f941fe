// codec_bvol.hip -- blind volume payloads (include/codec_tcc_blind_vol.h; specification:
// tests/pee_blind_volume_spec.py): one bitstream planned across a stack of blind stegos,
// each of which carries a 192-bit frame that names its place in the stream.
//
// Embed, all on one stream, no host round trip (the blind kernels are codec_blind.hip's):
//   k_blind_rows_auto   the one pass over the covers: the row table at every T
//   k_blind_plan_auto   the capacity curve [B][tmax] from that table (0 user bits)
//   k_bvol_plan         one workgroup of 1024 threads: c = max(curve - 192, 0), column sums per T,
//                       T*, a block scan of c at T* in rounds of 1024 with a carry, n_b and off_b in
//                       codec_tcc_vol.h's closed forms; lengths 192 + n_b, the skip marks, the frames,
//                       the info record.  No atomics.
//   k_bvol_rows         one thread per user-row word: the three frame words, then the share as a
//                       funnel shift of two stream words; a skipped slice's row is zero.
//   k_blind_plan_auto   again over the same table, on the lengths: T per carrier, skipped slices refused
//   k_blind_splice, the ROI embed, k_blind_pack with flag bit 2.
// Decode: the blind extract (skipped slices copied through), then
//   k_bvol_order        one workgroup: the frames judged, each carrier into its index slot and read
//                       back after the barrier, a running maximum of off + n over the slots (overlap,
//                       gaps), the slot tables and the info record.
//   k_bvol_gather       one thread per stream word: a binary search for the slot by offset, then a walk.
// Every value read back from device memory is clamped to its row, slice or table.
#include "codec_blind_int.h"
#include "codec_tcc_blind_vol.h"

#include <limits.h>

#include <algorithm>

#define BV_NT 1024
#define BV_FW (CODEC_PEE_BVOL_FRAME_BITS / 64)   // the frame's 64-bit row words: 3
#define BV_SLOTS 65536
#define BV_NMAX 0x7FFFFFFFLL

struct BvWs {
    BlWs bl;
    size_t curve, lens, skip, rows, soff, sn, sb, total;
};
static BvWs bv_ws(const codec_pee_params* P, size_t base, int tmax) {
    BvWs L;
    L.bl = bl_ws(P, base, tmax);
    const size_t B = (size_t)P->B;
    size_t o = L.bl.total;
    L.curve = o; o += align_up(B * (size_t)tmax * 4, 256);
    L.lens = o; o += align_up(B * 4, 256);
    L.skip = o; o += align_up(B * 4, 256);
    L.rows = o; o += align_up(B * (size_t)P->payload_words * 8, 256);
    L.soff = o; o += (size_t)BV_SLOTS * 4;
    L.sn = o; o += (size_t)BV_SLOTS * 4;
    L.sb = o; o += (size_t)BV_SLOTS * 4;
    L.total = o;
    return L;
}

// c[b][T-1] of a curve entry: the capacity past the frame, clamped to the slice's candidates
__device__ __forceinline__ u64 bv_cap(int32_t curve, uint32_t capmax) {
    return curve >= CODEC_PEE_BVOL_FRAME_BITS ? (u64)min((uint32_t)(curve - CODEC_PEE_BVOL_FRAME_BITS), capmax) : 0ull;
}

__device__ __forceinline__ u64 bv_scan_round(u64 x, u64* sh, u64& carry) {
    u64 tot;
    const u64 ex = block_excl_scan64<BV_NT>(x, sh, &tot);
    const u64 r = carry + ex;
    carry += tot;
    return r;
}

__global__ __launch_bounds__(BV_NT) void k_bvol_plan(const int32_t* __restrict__ curve, int B, int tmax, uint32_t capmax,
                                                     u64 nbits, int policy, uint32_t volume_id, uint32_t word2,
                                                     uint32_t stream_crc, int32_t* __restrict__ n_out,
                                                     int32_t* __restrict__ off_out, int32_t* __restrict__ lengths,
                                                     int32_t* __restrict__ skip, uint32_t* __restrict__ frames,
                                                     int32_t* __restrict__ info) {
    __shared__ u64 s_scan[BV_NT / 64 + 1];
    __shared__ u64 s_part[BV_NT / 64][CODEC_PEE_BLIND_TMAX];
    __shared__ u64 s_sum[CODEC_PEE_BLIND_TMAX];
    __shared__ int s_t, s_status;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    tmax = min(max(tmax, 1), CODEC_PEE_BLIND_TMAX);
    // lanes of one wave: tp columns (the power of two >= tmax) by 64 / tp rows
    int tp = 1;
    while (tp < tmax) tp <<= 1;
    const int col = lane & (tp - 1), sub = lane / tp, rpw = 64 / tp;
    u64 acc = 0;
    if (col < tmax)
        for (long long r = (long long)wv * rpw + sub; r < B; r += (long long)(BV_NT / 64) * rpw)
            acc += bv_cap(curve[(size_t)r * tmax + col], capmax);
    for (int o = 32; o >= tp; o >>= 1) acc += __shfl_xor(acc, o, 64);   // the lanes of one column
    if (lane < tp && lane < CODEC_PEE_BLIND_TMAX) s_part[wv][lane] = acc;
    __syncthreads();
    if (tid < tmax) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < BV_NT / 64; ++w) s += s_part[w][tid];
        s_sum[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int t = 1;
        while (t <= tmax && s_sum[t - 1] < nbits) ++t;
        s_status = t > tmax;
        s_t = t > tmax ? tmax : t;
    }
    __syncthreads();
    const int T = s_t;
    const bool refused = s_status != 0;
    const u64 N = nbits, PB = s_sum[T - 1];
    u64 carry = 0, carriers = 0;
    for (int base = 0; base < B; base += BV_NT) {
        const int b = base + tid;
        const u64 c = b < B ? bv_cap(curve[(size_t)b * tmax + (T - 1)], capmax) : 0ull;
        const u64 Pb = bv_scan_round(c, s_scan, carry);
        u64 off = 0, n = 0;
        if (b < B && !refused) {
            if (policy == 1) {
                off = min(N, Pb);
                n = min(c, N - off);
            } else {
                off = PB ? N * Pb / PB : 0ull;   // N, P < 2^31: the products stay below 2^62
                n = (PB ? N * (Pb + c) / PB : 0ull) - off;
            }
        }
        (void)bv_scan_round(n > 0 ? 1ull : 0ull, s_scan, carriers);
        if (b < B) {
            n_out[b] = (int32_t)n;
            off_out[b] = (int32_t)off;
            lengths[b] = n > 0 ? CODEC_PEE_BVOL_FRAME_BITS + (int32_t)n : 0;
            skip[b] = n > 0 ? 0 : 1;
            uint32_t* f = frames + (size_t)b * CODEC_PEE_BVOL_FRAME_WORDS;
            const bool on = n > 0;
            f[0] = on ? volume_id : 0u; f[1] = on ? (uint32_t)b : 0u; f[2] = on ? word2 : 0u;
            f[3] = on ? (uint32_t)off : 0u; f[4] = on ? (uint32_t)N : 0u; f[5] = on ? stream_crc : 0u;
        }
        if (B - base <= BV_NT) break;   // (base + BV_NT could pass INT_MAX)
    }
    if (tid == 0) {
        info[0] = s_status; info[1] = T; info[2] = (int32_t)PB; info[3] = (int32_t)s_sum[tmax - 1];
        info[4] = (int32_t)carriers; info[5] = (int32_t)N; info[6] = policy; info[7] = B;
    }
}

// grid (row words / 256, B): user row b = frame || stream bits [off_b, off_b + n_b), zero above; skipped: zero
__global__ __launch_bounds__(256) void k_bvol_rows(const u64* __restrict__ bits, u64 stream_words,
                                                   const int32_t* __restrict__ n, const int32_t* __restrict__ off,
                                                   const int32_t* __restrict__ skip, const uint32_t* __restrict__ frames,
                                                   int uw, u64* __restrict__ rows) {
    const int b = blockIdx.y;
    const int w = (int)blockIdx.x * 256 + threadIdx.x;
    if (w >= uw) return;
    u64 v = 0;
    if (!skip[b]) {
        if (w < BV_FW) {
            const uint32_t* f = frames + (size_t)b * CODEC_PEE_BVOL_FRAME_WORDS;
            v = (u64)f[2 * w] | ((u64)f[2 * w + 1] << 32);
        } else {
            const long long k = w - BV_FW;
            const long long nb = min((long long)max(n[b], 0), 64ll * (uw - BV_FW));
            if (64ll * k < nb) {
                const long long p = (long long)max(off[b], 0) + 64ll * k;
                const u64 idx = (u64)p >> 6;
                const int sh = (int)(p & 63);
                const long long rem = min(nb - 64ll * k, 64ll);
                v = (idx < stream_words ? bits[idx] : 0ull) >> sh;
                if (sh && 64 - sh < rem) v |= (idx + 1 < stream_words ? bits[idx + 1] : 0ull) << (64 - sh);
                if (rem < 64) v &= (1ull << rem) - 1ull;
            }
        }
    }
    rows[(size_t)b * uw + w] = v;
}

// ---- decode
__device__ __forceinline__ uint32_t bv_frame_word(const u64* __restrict__ row, int k) {
    const u64 w = row[k >> 1];
    return (k & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
}
// the share's length a header states, clamped to the user row
__device__ __forceinline__ long long bv_share_bits(const uint32_t* __restrict__ hdr, int b, int uw) {
    return min(max((long long)hdr[8 * b + 2] - CODEC_PEE_BVOL_FRAME_BITS, 0LL), 64LL * (uw - BV_FW));
}

// exclusive running maximum over the threads of this round and the rounds before it (sh: BV_NT / 64 words)
__device__ __forceinline__ uint32_t bv_max_round(uint32_t x, uint32_t* sh, uint32_t& carry) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, y);
    }
    uint32_t ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0u;
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint32_t pre = carry, tot = carry;
    for (int w = 0; w < BV_NT / 64; ++w) {
        const uint32_t v = sh[w];
        if (w < wv) pre = max(pre, v);
        tot = max(tot, v);
    }
    __syncthreads();   // sh reusable
    carry = tot;
    return max(pre, ex);
}

// one workgroup.  rows [B][uw]: the user rows of the extract; slot tables of BV_SLOTS entries.
__global__ __launch_bounds__(BV_NT) void k_bvol_order(const u64* __restrict__ rows, int uw, const uint32_t* __restrict__ hdr,
                                                      const int32_t* __restrict__ skip, int B, int32_t* __restrict__ soff,
                                                      int32_t* __restrict__ sn, int32_t* __restrict__ sb,
                                                      int32_t* __restrict__ info, int32_t* __restrict__ table) {
    __shared__ uint32_t s_sh[BV_NT / 64];
    __shared__ int s_first[BV_NT / 64];
    __shared__ u64 s_gap[BV_NT / 64];
    __shared__ int s_flags;   // 1 mixed, 2 out of range / duplicate / overlap, 4 gap
    __shared__ int s_count[BV_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the first carrier and the carriers' count
    int first = INT_MAX, count = 0;
    for (int b = tid; b < B; b += BV_NT)
        if (!(skip && skip[b])) { first = min(first, b); ++count; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        first = min(first, __shfl_xor(first, o, 64));
        count += __shfl_xor(count, o, 64);
    }
    if (lane == 0) { s_first[wv] = first; s_count[wv] = count; }
    if (tid == 0) s_flags = 0;
    __syncthreads();
    first = INT_MAX; count = 0;
    for (int w = 0; w < BV_NT / 64; ++w) { first = min(first, s_first[w]); count += s_count[w]; }
    uint32_t ref[CODEC_PEE_BVOL_FRAME_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (first < B)
        for (int k = 0; k < CODEC_PEE_BVOL_FRAME_WORDS; ++k) ref[k] = bv_frame_word(rows + (size_t)first * uw, k);
    const int Bf = (int)(ref[2] & 0xFFFFu);
    const bool ref_ok = first < B && Bf >= 1 && ref[4] >= 1u && (long long)ref[4] <= BV_NMAX;
    const uint32_t N = ref_ok ? ref[4] : 0u;
    const int nslots = ref_ok ? Bf : 0;
    for (int s = tid; s < nslots; s += BV_NT) sb[s] = -1;
    __syncthreads();
    // every carrier into its slot
    int flags = 0;
    for (int base = 0; base < B; base += BV_NT) {
        const int b = base + tid;
        bool took = false;
        uint32_t idx = 0, off = 0;
        long long nb = 0;
        if (b < B && !(skip && skip[b])) {
            const u64* row = rows + (size_t)b * uw;
            idx = bv_frame_word(row, 1);
            off = bv_frame_word(row, 3);
            nb = bv_share_bits(hdr, b, uw);
            const bool same = bv_frame_word(row, 0) == ref[0] && bv_frame_word(row, 2) == ref[2] &&
                              bv_frame_word(row, 4) == ref[4] && bv_frame_word(row, 5) == ref[5];
            if (!same || !ref_ok) flags |= 1;
            else if (idx >= (uint32_t)nslots || (long long)off + nb > (long long)N) flags |= 2;
            else { took = true; sb[idx] = b; }
        }
        __syncthreads();   // the slots written in this round are visible to the workgroup
        if (took && sb[idx] != b) { flags |= 2; took = false; }   // another carrier of this round has the index
        if (b < B) {
            int32_t* t = table + 4 * (size_t)b;
            t[0] = (int32_t)idx; t[1] = (int32_t)off; t[2] = (int32_t)nb; t[3] = took ? 1 : 0;
        }
        __syncthreads();
        if (B - base <= BV_NT) break;
    }
    // a carrier of an earlier round that lost its slot to a later one
    for (int b = tid; b < B; b += BV_NT) {
        const int32_t* t = table + 4 * (size_t)b;
        if (t[3] && sb[min(max(t[0], 0), BV_SLOTS - 1)] != b) flags |= 2;
    }
    // the slots in index order: running maximum of off + n
    uint32_t carry = 0;
    u64 gap = ~0ull;   // (first bit << 32 | end) of the lowest gap
    for (int base = 0; base < nslots; base += BV_NT) {
        const int s = base + tid;
        int b = s < nslots ? sb[s] : -1;
        if (b >= B) b = -1;
        uint32_t off = 0, nb = 0;
        if (b >= 0) {
            off = min(bv_frame_word(rows + (size_t)b * uw, 3), N);
            nb = (uint32_t)min(bv_share_bits(hdr, b, uw), (long long)(N - off));
        }
        const uint32_t prev = bv_max_round(b >= 0 ? off + nb : 0u, s_sh, carry);
        if (b >= 0) {
            if (off < prev) flags |= 2;
            if (off > prev) { flags |= 4; gap = min(gap, ((u64)prev << 32) | off); }
        }
        if (s < nslots) {
            soff[s] = (int32_t)(b >= 0 ? off : prev);
            sn[s] = (int32_t)nb;
        }
    }
    if (ref_ok && carry < N) { flags |= 4; gap = min(gap, ((u64)carry << 32) | N); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        flags |= __shfl_xor(flags, o, 64);
        gap = min(gap, (u64)__shfl_xor(gap, o, 64));
    }
    if (lane == 0) { atomicOr(&s_flags, flags); s_gap[wv] = gap; }   // an LDS atomic
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < BV_NT / 64; ++w) gap = min(gap, s_gap[w]);
        const int f = s_flags;
        const int status = count == 0 ? CODEC_PEE_BVOL_NO_CARRIER : (f & 1) ? CODEC_PEE_BVOL_MIXED
                           : (f & 2) ? CODEC_PEE_BVOL_OVERLAP : (f & 4) ? CODEC_PEE_BVOL_GAP : CODEC_PEE_BVOL_OK;
        const bool g = status == CODEC_PEE_BVOL_GAP && gap != ~0ull;
        info[0] = status; info[1] = count; info[2] = (int32_t)N; info[3] = (int32_t)ref[2]; info[4] = (int32_t)ref[0];
        info[5] = g ? (int32_t)(gap >> 32) : 0; info[6] = g ? (int32_t)(gap & 0xFFFFFFFFull) : 0; info[7] = (int32_t)ref[5];
    }
}

__global__ __launch_bounds__(256) void k_bvol_gather(const u64* __restrict__ rows, int uw, int B,
                                                     const int32_t* __restrict__ info, const int32_t* __restrict__ soff,
                                                     const int32_t* __restrict__ sn, const int32_t* __restrict__ sb,
                                                     u64* __restrict__ bits, u64 stream_words) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= stream_words) return;
    const int status = info[0];
    const bool usable = status == CODEC_PEE_BVOL_OK || status == CODEC_PEE_BVOL_GAP;
    const int nslots = usable ? min(max(info[3] & 0xFFFF, 0), BV_SLOTS - 1) : 0;
    const long long N = max(info[2], 0);
    const long long pos = (long long)(j << 6), stop = min(pos + 64, N);
    u64 v = 0;
    if (nslots > 0 && pos < N) {
        int lo = 0, hi = nslots;   // the last slot with soff <= pos, or slot 0
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (soff[mid] <= pos) lo = mid; else hi = mid;
        }
        long long cur = pos;
        for (int s = lo; s < nslots && cur < stop; ++s) {
            const int b = sb[s];
            const long long o = min((long long)max(soff[s], 0), N);
            const long long n = min((long long)max(sn[s], 0), min(N - o, 64LL * (uw - BV_FW)));
            if (b < 0 || b >= B || n <= 0 || o + n <= cur) continue;
            if (o >= stop) break;
            if (o > cur) cur = o;   // uncovered bits stay zero
            const int cnt = (int)(min(o + n, stop) - cur);
            const long long r = cur - o;
            const long long wi = BV_FW + (r >> 6);
            const int sh = (int)(r & 63);
            const u64* row = rows + (size_t)b * uw;
            u64 x = (wi < uw ? row[wi] : 0ull) >> sh;
            if (sh && 64 - sh < cnt) x |= (wi + 1 < uw ? row[wi + 1] : 0ull) << (64 - sh);
            if (cnt < 64) x &= (1ull << cnt) - 1ull;
            v |= x << (int)(cur - pos);
            cur += cnt;
        }
    }
    bits[j] = v;
}

// ====================================================================== host side
static long long bv_nc(const codec_pee_params* P) { return (long long)(P->H / 2) * (P->W / 2); }

// the checks every entry shares, behind codec_tcc_blind.h's
static int bv_check(const codec_pee_params* P, int32_t tmax, int32_t max_entries, size_t* base, const char* who) {
    int rc = blind_check(P, max_entries, true, base, who, tmax);
    if (rc) return rc;
    if (P->B > CODEC_PEE_BVOL_MAX_B) return set_err(CODEC_EINVAL, "%s: B must be <= 65535 (the frame's 16 bits)", who);
    if ((long long)P->B * bv_nc(P) > BV_NMAX) return set_err(CODEC_EINVAL, "%s: B (H/2) (W/2) must be <= 2^31 - 1", who);
    if (P->payload_words < BV_FW + 1) return set_err(CODEC_EINVAL, "%s: payload_words must be >= 4 (the frame and a share word)", who);
    return 0;
}
static int bv_check_plan(int64_t nbits, int32_t policy, const char* who) {
    if (nbits < 1 || nbits > BV_NMAX) return set_err(CODEC_EINVAL, "%s: nbits must be in 1..2^31 - 1", who);
    if (policy != 0 && policy != 1) return set_err(CODEC_EINVAL, "%s: policy must be 0 (even) or 1 (fill)", who);
    return 0;
}
static int bv_check_rows(int32_t user_words, const char* who) {
    if (user_words < BV_FW || user_words > (1 << 24)) return set_err(CODEC_EINVAL, "%s: user_words must be in 3..2^24", who);
    return 0;
}
static int bv_check_stream(int64_t stream_words, const char* who) {
    if (stream_words < 0 || stream_words > (1LL << 25)) return set_err(CODEC_EINVAL, "%s: stream_words must be in 0..2^25", who);
    return 0;
}

static int bv_launch_plan(const codec_pee_params* P, const int32_t* curve, int32_t tmax, int64_t nbits, int32_t policy,
                          uint32_t volume_id, int32_t frame_crc, uint32_t stream_crc, int32_t* n_out, int32_t* off_out,
                          int32_t* lengths, int32_t* skip, uint32_t* frames, int32_t* info, hipStream_t st) {
    const uint32_t word2 = (uint32_t)P->B | (frame_crc ? CODEC_PEE_BVOL_FRAME_CRC : 0u);
    ProfScope prof(st, CODEC_K_BVOL_PLAN);
    hipLaunchKernelGGL(k_bvol_plan, dim3(1), dim3(BV_NT), 0, st, curve, (int)P->B, (int)tmax, (uint32_t)bv_nc(P), (u64)nbits,
                       (int)policy, volume_id, word2, frame_crc ? stream_crc : 0u, n_out, off_out, lengths, skip, frames, info);
    LAUNCH_CHECK("k_bvol_plan");
    return 0;
}

static int bv_launch_order(const codec_pee_params* P, const BvWs& L, const uint64_t* rows, int32_t user_words,
                           const uint32_t* hdr, const int32_t* skip, int32_t* info, int32_t* table, char* ws, hipStream_t st) {
    ProfScope prof(st, CODEC_K_BVOL_ORDER);
    hipLaunchKernelGGL(k_bvol_order, dim3(1), dim3(BV_NT), 0, st, reinterpret_cast<const u64*>(rows), (int)user_words, hdr, skip,
                       (int)P->B, reinterpret_cast<int32_t*>(ws + L.soff), reinterpret_cast<int32_t*>(ws + L.sn),
                       reinterpret_cast<int32_t*>(ws + L.sb), info, table);
    LAUNCH_CHECK("k_bvol_order");
    return 0;
}

static int bv_launch_gather(const codec_pee_params* P, const BvWs& L, const uint64_t* rows, int32_t user_words,
                            const int32_t* info, uint64_t* bitstream, int64_t stream_words, char* ws, hipStream_t st) {
    if (stream_words <= 0) return 0;
    ProfScope prof(st, CODEC_K_BVOL_GATHER);
    hipLaunchKernelGGL(k_bvol_gather, dim3((unsigned)((stream_words + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const u64*>(rows), (int)user_words, (int)P->B, info,
                       reinterpret_cast<const int32_t*>(ws + L.soff), reinterpret_cast<const int32_t*>(ws + L.sn),
                       reinterpret_cast<const int32_t*>(ws + L.sb), reinterpret_cast<u64*>(bitstream), (u64)stream_words);
    LAUNCH_CHECK("k_bvol_gather");
    return 0;
}

extern "C" {

size_t codec_pee_blind_volume_workspace_bytes(const codec_pee_params* P, int32_t tmax, int32_t max_entries) {
    size_t base = 0;
    if (bv_check(P, tmax, max_entries, &base, "codec_pee_blind_volume_workspace_bytes")) return 0;
    return bv_ws(P, base, tmax).total;
}

int codec_pee_blind_volume_plan(const codec_pee_params* P, const int32_t* curve, int32_t tmax, int64_t nbits,
                                int32_t policy, uint32_t volume_id, int32_t frame_crc, uint32_t stream_crc,
                                int32_t* n_out, int32_t* off_out, int32_t* lengths_out, int32_t* skip_out,
                                uint32_t* frames_out, int32_t* info, void* stream) {
    const char* who = "codec_pee_blind_volume_plan";
    size_t base = 0;
    int rc = bv_check(P, tmax, 0, &base, who);
    if (rc) return rc;
    if ((rc = bv_check_plan(nbits, policy, who))) return rc;
    if (!curve || !n_out || !off_out || !lengths_out || !skip_out || !frames_out || !info)
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    return bv_launch_plan(P, curve, tmax, nbits, policy, volume_id, frame_crc, stream_crc, n_out, off_out, lengths_out,
                          skip_out, frames_out, info, as_stream(stream));
}

int codec_pee_blind_volume_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                                 int64_t nbits, int32_t policy, int32_t tmax, int32_t max_entries, uint32_t volume_id,
                                 int32_t frame_crc, uint32_t stream_crc, const uint32_t* cover_crc, int32_t* n_out,
                                 int32_t* off_out, uint32_t* frames_out, int32_t* info, int32_t* slice_info,
                                 int32_t* t_out, codec_pee_meta* meta, uint64_t* lm, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_volume_embed";
    size_t base = 0;
    int rc = bv_check(P, tmax, max_entries, &base, who);
    if (rc) return rc;
    if ((rc = bv_check_plan(nbits, policy, who))) return rc;
    if (!cover || !stego || !bitstream || !n_out || !off_out || !frames_out || !info || !slice_info || !t_out || !meta ||
        !lm || !workspace)
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    if (cover == stego) return set_err(CODEC_EINVAL, "%s: out of place only (cover == stego)", who);
    const BvWs L = bv_ws(P, base, tmax);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* curve = reinterpret_cast<int32_t*>(ws + L.curve);
    int32_t* lengths = reinterpret_cast<int32_t*>(ws + L.lens);
    int32_t* skip = reinterpret_cast<int32_t*>(ws + L.skip);
    uint64_t* rows = reinterpret_cast<uint64_t*>(ws + L.rows);
    const int uw = P->payload_words;
    // the one pass over the covers, then the curve: the capacities are the format's own (no row bound)
    if ((rc = blind_rows_auto(P, L.bl, cover, tmax, ws, st))) return rc;
    if ((rc = blind_plan_table(P, L.bl, nullptr, nullptr, INT_MAX, 0, 1LL << 40, tmax, max_entries, slice_info, t_out, curve,
                               ws, st)))
        return rc;
    if ((rc = bv_launch_plan(P, curve, tmax, nbits, policy, volume_id, frame_crc, stream_crc, n_out, off_out, lengths, skip,
                             frames_out, info, st)))
        return rc;
    {
        ProfScope prof(st, CODEC_K_BVOL_ROWS);
        dim3 grid((unsigned)((uw + 255) / 256), (unsigned)P->B);
        hipLaunchKernelGGL(k_bvol_rows, grid, dim3(256), 0, st, reinterpret_cast<const u64*>(bitstream),
                           (u64)((nbits + 63) / 64), n_out, off_out, skip, frames_out, uw, reinterpret_cast<u64*>(rows));
        LAUNCH_CHECK("k_bvol_rows");
    }
    // T per carrier over the same table: the covers are not read again
    if ((rc = blind_plan_table(P, L.bl, lengths, skip, (int)std::min(64LL * uw, (long long)INT_MAX), 0, 64LL * P->payload_words, tmax, max_entries, slice_info,
                               t_out, nullptr, ws, st)))
        return rc;
    return blind_embed_planned(P, L.bl, cover, stego, rows, uw, nullptr, cover_crc,
                               CODEC_PEE_BLIND_FLAG_VOLUME | (cover_crc ? CODEC_PEE_BLIND_FLAG_CRC : 0u), slice_info, meta, lm,
                               workspace, workspace_bytes, stream);
}

int codec_pee_blind_volume_order(const codec_pee_params* P, const uint64_t* rows, int32_t user_words,
                                 const uint32_t* hdr, const int32_t* skip, int32_t* info, int32_t* table_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_volume_order";
    size_t base = 0;
    int rc = bv_check(P, 1, 0, &base, who);
    if (rc) return rc;
    if ((rc = bv_check_rows(user_words, who))) return rc;
    if (!rows || !hdr || !info || !table_out || !workspace) return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    const BvWs L = bv_ws(P, base, 1);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    return bv_launch_order(P, L, rows, user_words, hdr, skip, info, table_out, static_cast<char*>(workspace), as_stream(stream));
}

int codec_pee_blind_volume_gather(const codec_pee_params* P, const uint64_t* rows, int32_t user_words,
                                  const int32_t* info, uint64_t* bitstream, int64_t stream_words, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "codec_pee_blind_volume_gather";
    size_t base = 0;
    int rc = bv_check(P, 1, 0, &base, who);
    if (rc) return rc;
    if ((rc = bv_check_rows(user_words, who))) return rc;
    if ((rc = bv_check_stream(stream_words, who))) return rc;
    if (!rows || !info || !workspace || (!bitstream && stream_words > 0))
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    const BvWs L = bv_ws(P, base, 1);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    return bv_launch_gather(P, L, rows, user_words, info, bitstream, stream_words, static_cast<char*>(workspace),
                            as_stream(stream));
}

int codec_pee_blind_volume_extract(const codec_pee_params* P, const void* stego, const uint32_t* hdr,
                                   const codec_pee_meta* meta, const int32_t* skip, void* cover_out,
                                   uint64_t* rows_out, int32_t user_words, uint64_t* bitstream, int64_t stream_words,
                                   int32_t* info, int32_t* table_out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const char* who = "codec_pee_blind_volume_extract";
    size_t base = 0;
    int rc = bv_check(P, 1, 0, &base, who);
    if (rc) return rc;
    if ((rc = bv_check_rows(user_words, who))) return rc;
    if ((rc = bv_check_stream(stream_words, who))) return rc;
    if (!stego || !hdr || !meta || !cover_out || !rows_out || !info || !table_out || !workspace ||
        (!bitstream && stream_words > 0))
        return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    if (stego == cover_out) return set_err(CODEC_EINVAL, "%s: out of place only (stego == cover_out)", who);
    const BvWs L = bv_ws(P, base, 1);
    if (workspace_bytes < L.total) return set_err(CODEC_EINVAL, "%s: workspace too small", who);
    if ((rc = pee_workspace_enter(P, workspace, stream))) return rc;
    char* ws = static_cast<char*>(workspace);
    if ((rc = blind_extract_launch(P, L.bl, stego, hdr, meta, skip, cover_out, rows_out, user_words, workspace, workspace_bytes,
                                   stream)))
        return rc;
    if ((rc = bv_launch_order(P, L, rows_out, user_words, hdr, skip, info, table_out, ws, as_stream(stream)))) return rc;
    return bv_launch_gather(P, L, rows_out, user_words, info, bitstream, stream_words, ws, as_stream(stream));
}

}  // extern "C"

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
// Every kernel clamps what it reads from device memory to the slice, the row and the map.
#include "codec_common.h"
#include "codec_tcc_blind.h"

#include <limits.h>

#include <algorithm>

#define BL_HDR_BITS 192
#define BL_PAD 0xFFFFFFFFu
#define BL_ROWS_PER_WAVE 4
#define BL_ROWS_PER_WG (4 * BL_ROWS_PER_WAVE)
#define BL_U 4

struct BlWs {
    size_t rows, rect, lens, ts, gs, lm, pay, total;
};
// the layout behind the codec_pee workspace of P (base = codec_pee_workspace_bytes(P) > 0)
static BlWs bl_ws(const codec_pee_params* P, size_t base) {
    BlWs L;
    const size_t B = (size_t)P->B;
    size_t o = align_up(base, 256);
    L.rows = o; o += align_up(B * (size_t)(P->H / 2 > 0 ? P->H / 2 : 1) * 8, 256);
    L.rect = o; o += align_up(B * 16, 256);
    L.lens = o; o += align_up(B * 4, 256);
    L.ts = o; o += align_up(B * 4, 256);
    L.gs = o; o += align_up(B * 4, 256);
    L.lm = o; o += align_up(B * (size_t)P->lm_words * 8, 256);
    L.pay = o; o += align_up(B * (size_t)P->payload_words * 8, 256);
    L.total = o;
    return L;
}

__device__ __forceinline__ int bl_med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), a + b - c)); }

template <typename V> __device__ __forceinline__ uint32_t bl_px(const V& v, int e);
template <> __device__ __forceinline__ uint32_t bl_px<uint4>(const uint4& v, int e) {
    const uint32_t w = e < 2 ? v.x : (e < 4 ? v.y : (e < 6 ? v.z : v.w));
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
template <> __device__ __forceinline__ uint32_t bl_px<uint2>(const uint2& v, int e) {
    return ((e < 4 ? v.x : v.y) >> (8 * (e & 3))) & 0xFFu;
}

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

// one workgroup per slice.  lengths NULL: 0 user bits each; a length is clamped to 0 .. user_bits.
__global__ __launch_bounds__(256) void k_blind_plan(const uint2* __restrict__ rows, const int32_t* __restrict__ lengths,
                                                    int user_bits, int H, int W, int thr, int max_entries,
                                                    long long row_bits, int32_t* __restrict__ info,
                                                    int32_t* __restrict__ rect, int32_t* __restrict__ lens,
                                                    int32_t* __restrict__ ts, int32_t* __restrict__ gs) {
    __shared__ uint32_t sh[256 / 64 + 1];
    __shared__ u64 s_first;
    __shared__ int s_cap;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hc = H / 2;
    const long long n_user = lengths ? (long long)min(max(lengths[b], 0), user_bits) : 0;
    if (tid == 0) { s_first = ~0ull; s_cap = -1; }
    __syncthreads();
    uint32_t cap0 = 0, uns0 = 0;
    for (int c0 = 0; c0 < hc; c0 += 256) {
        const int i = c0 + tid;
        const uint2 v = i < hc ? rows[(size_t)b * hc + i] : make_uint2(0u, 0u);
        uint32_t tc, tu;
        const uint32_t cap = cap0 + block_excl_scan<256>(v.x, sh, &tc) + v.x;   // through row i
        const uint32_t uns = uns0 + block_excl_scan<256>(v.y, sh, &tu) + v.y;
        if (i < hc) {
            const long long side = BL_HDR_BITS + 32LL * uns;
            const long long room = (long long)cap - side;
            const long long rr = (side + 2LL * W - 1) / (2LL * W);
            if (i < hc - rr && uns <= (uint32_t)max_entries && side <= row_bits && room >= 0)
                atomicMax(&s_cap, (int)min(room, row_bits - side));
            if (room >= n_user) atomicMin(&s_first, ((u64)(uint32_t)i << 32) | uns);
        }
        cap0 += tc;
        uns0 += tu;
    }
    __syncthreads();
    if (tid != 0) return;
    int status = 0, E = 0, n_side = 0, istar = -1, y0 = 0;
    if (s_first == ~0ull) {
        status = 1;
    } else {
        istar = (int)(s_first >> 32);
        const long long e = (long long)(s_first & 0xFFFFFFFFull);
        const long long side = BL_HDR_BITS + 32 * e;
        const long long rr = (side + 2LL * W - 1) / (2LL * W);
        E = (int)min(e, (long long)INT_MAX);
        if (istar >= hc - rr) status = 1;
        else if (e > max_entries) status = 2;
        else if (side + n_user > row_bits) status = 1;   // a row narrower than the call's lengths: the host sizes it
        else { n_side = (int)side; y0 = 2 * (hc - (int)rr); }
    }
    int32_t* I = info + (size_t)b * CODEC_PEE_BLIND_INFO_WORDS;
    I[0] = status; I[1] = (int)n_user; I[2] = E; I[3] = n_side; I[4] = -1; I[5] = y0; I[6] = istar; I[7] = s_cap;
    const bool ok = status == 0;
    rect[4 * b] = ok ? y0 : 0; rect[4 * b + 1] = 0; rect[4 * b + 2] = ok ? H : 0; rect[4 * b + 3] = ok ? W : 0;
    lens[b] = ok ? n_side + (int)n_user : 0;
    ts[b] = thr;
    gs[b] = CODEC_PEE_GATE_MAX;
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

// payload row = displaced LSBs (side bit i = bit 0 of pixel npx - 1 - i) || user bits; grid (row words / 256, B)
template <typename T>
__global__ __launch_bounds__(256) void k_blind_splice(const T* __restrict__ img, long long npx,
                                                      const u64* __restrict__ user, int user_words,
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
            const long long q = lo - n_side;   // the user bit at position lo (negative: the row's first user bit lies inside)
            if (q >= 0) {
                const int sh = (int)(q & 63);
                v |= bl_user_word(row, q >> 6, n_user) >> sh;
                if (sh) v |= bl_user_word(row, (q >> 6) + 1, n_user) << (64 - sh);
            } else {
                v |= bl_user_word(row, 0, n_user) << (int)(-q);
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

// one workgroup per slice, after the ROI embed: header, entries, padding; info's `end`
template <typename T>
__global__ __launch_bounds__(256) void k_blind_pack(T* __restrict__ stego, long long npx, int nc, int thr, int maxval,
                                                    const codec_pee_meta* __restrict__ meta, const u64* __restrict__ lm,
                                                    int lm_words, const uint32_t* __restrict__ crc,
                                                    int32_t* __restrict__ info) {
    __shared__ uint32_t sh[256 / 64 + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* I = info + (size_t)b * CODEC_PEE_BLIND_INFO_WORDS;
    if (I[0] != 0) return;   // refused: the ROI embed copied the cover through (length 0, no rectangle)
    const int E = I[2];
    const int end = min(max(meta[b].end, -1), min(nc, 64 * lm_words) - 1);
    T* px = stego + (size_t)b * npx;
    if (tid < CODEC_PEE_BLIND_HDR_WORDS) {
        const uint32_t hw[CODEC_PEE_BLIND_HDR_WORDS] = {
            CODEC_PEE_BLIND_MAGIC,
            (uint32_t)thr | ((crc ? (uint32_t)CODEC_PEE_BLIND_FLAG_CRC : 0u) << 8) | ((uint32_t)maxval << 16),
            (uint32_t)I[1], (uint32_t)E, (uint32_t)end, crc ? crc[b] : 0u};
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
                                                       u64* __restrict__ lm, int lm_words) {
    const int b = blockIdx.y;
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    const BlHdr h = bl_hdr(hdr, b, npx, row_bits, nc);
    if (e >= h.E) return;
    const uint32_t idx = bl_get_word(stego + (size_t)b * npx, npx, BL_HDR_BITS + 32LL * e);
    if (idx == BL_PAD || (long long)idx > (long long)h.end || idx >= (uint32_t)nc || (idx >> 6) >= (uint32_t)lm_words) return;
    atomicOr(reinterpret_cast<u64*>(lm) + (size_t)b * lm_words + (idx >> 6), 1ull << (idx & 63));
}

// after the ROI extract: thread t restores side bit t and writes user word t; grid (max(bits, words) / 256, B)
template <typename T>
__global__ __launch_bounds__(256) void k_blind_restore(T* __restrict__ cover, long long npx, int nc, long long row_bits,
                                                       const uint32_t* __restrict__ hdr, const u64* __restrict__ rows,
                                                       int row_words, u64* __restrict__ out, int user_words) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const BlHdr h = bl_hdr(hdr, b, npx, row_bits, nc);
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

// the checks every entry shares; `ws`: the entry takes the workspace
static int blind_check(const codec_pee_params* P, int32_t max_entries, bool ws, size_t* base, const char* who) {
    if (!P) return set_err(CODEC_EINVAL, "%s: params is NULL", who);
    if (max_entries < 0 || max_entries > CODEC_PEE_BLIND_MAX_ENTRIES)
        return set_err(CODEC_EINVAL, "%s: max_entries must be in 0..65536", who);
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

// row table and plan on the workspace's arrays (lengths NULL: 0 bits each)
static int blind_plan(const codec_pee_params* P, const BlWs& L, const void* cover, const int32_t* lengths, int user_bits,
                      long long row_bits, int32_t max_entries, int32_t* info, char* ws, hipStream_t st) {
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
    hipLaunchKernelGGL(k_blind_plan, dim3((unsigned)P->B), dim3(256), 0, st, rows, lengths, user_bits, P->H, P->W, P->T,
                       (int)max_entries, row_bits, info, reinterpret_cast<int32_t*>(ws + L.rect),
                       reinterpret_cast<int32_t*>(ws + L.lens), reinterpret_cast<int32_t*>(ws + L.ts),
                       reinterpret_cast<int32_t*>(ws + L.gs));
    LAUNCH_CHECK("k_blind_plan");
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
    return blind_plan(P, L, cover, lengths, INT_MAX, 1LL << 40, max_entries, info, static_cast<char*>(workspace),
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
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    if ((rc = blind_plan(P, L, cover, lengths, 64 * user_words, 64LL * P->payload_words, max_entries, info, ws, st))) return rc;
    u64* rows = reinterpret_cast<u64*>(ws + L.pay);
    const long long npx = (long long)P->H * P->W;
    {
        dim3 grid((unsigned)((P->payload_words + 255) / 256), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            hipLaunchKernelGGL(k_blind_splice<TT>, grid, dim3(256), 0, st, static_cast<const TT*>(cover), npx,
                               reinterpret_cast<const u64*>(payload), (int)user_words, info, rows, P->payload_words);
        });
        LAUNCH_CHECK("k_blind_splice");
    }
    rc = codec_pee_roi_embed(P, cover, stego, reinterpret_cast<const uint64_t*>(rows),
                             reinterpret_cast<const int32_t*>(ws + L.lens), reinterpret_cast<const int32_t*>(ws + L.ts),
                             reinterpret_cast<const int32_t*>(ws + L.gs), reinterpret_cast<const int32_t*>(ws + L.rect), meta,
                             lm, workspace, workspace_bytes, stream);
    if (rc) return rc;
    const int nc = (P->H / 2) * (P->W / 2);
    pee_pixel(P->bytes, [&](auto px) {
        using TT = decltype(px);
        hipLaunchKernelGGL(k_blind_pack<TT>, dim3((unsigned)P->B), dim3(256), 0, st, static_cast<TT*>(stego), npx, nc, P->T,
                           P->maxval, meta, reinterpret_cast<const u64*>(lm), P->lm_words, crc, info);
    });
    LAUNCH_CHECK("k_blind_pack");
    return 0;
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
                               hdr, lm, P->lm_words);
        });
        LAUNCH_CHECK("k_blind_scatter");
    }
    rc = codec_pee_roi_extract(P, stego, meta, reinterpret_cast<const uint64_t*>(lm), cover_out,
                               reinterpret_cast<uint64_t*>(rows), workspace, workspace_bytes, stream);
    if (rc) return rc;
    {
        const long long n = std::max(row_bits, (long long)user_words);
        dim3 grid((unsigned)((n + 255) / 256), (unsigned)P->B);
        pee_pixel(P->bytes, [&](auto px) {
            using TT = decltype(px);
            hipLaunchKernelGGL(k_blind_restore<TT>, grid, dim3(256), 0, st, static_cast<TT*>(cover_out), npx, nc, row_bits, hdr,
                               rows, P->payload_words, reinterpret_cast<u64*>(payload_out), (int)user_words);
        });
        LAUNCH_CHECK("k_blind_restore");
    }
    return 0;
}

}  // extern "C"

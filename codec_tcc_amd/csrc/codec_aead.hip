// codec_aead.hip -- keyed MED-PEE: ChaCha20 over payload rows, Poly1305 over covers and rows,
// the release step (include/codec_tcc_aead.h; the specification is tests/aead_spec.py).
//
// ChaCha20 (k_chacha20_rows, k_aead_release = the same kernel with the tag comparison in front
// of its stores).  The grid covers the (row, 64-byte block) pairs of the batch, so 256 rows of
// 1 KB and one row of 256 MB are the same launch.  Two layouts (A/B: profiles/r14/):
//   0  a lane owns a block: the 16 state words in 16 registers, eight 8-byte accesses at a
//      64-byte stride;
//   1  a quad owns a block, lane q holding column q (words q, 4+q, 8+q, 12+q): the column round
//      needs no lane traffic, the diagonal round is the same four quarter-rounds after rotating
//      rows 1..3 by 1..3 lanes with DPP quad_perm; a 4 x 4 transpose inside the quad (three more
//      quad_perm moves) then gives lane q words 4q .. 4q+3, i.e. 16 contiguous bytes per lane and
//      1 KB contiguous per wave access.
// Rotates are v_alignbit_b32.  Rows are 8-byte aligned only (row_words may be odd), so the
// accesses are 8 bytes wide.
//
// Poly1305, arithmetic mod p = 2^130 - 5 in five 26-bit limbs with 64-bit multiply-adds
// (v_mad_u64_u32) and the 5 r limbs precomputed (p13_mul).  The tag of slice b is
//     (sum_i m_i r^(N - i) mod p  +  s) mod 2^128,   i = 0 .. N-1,
// over its N = NA + NC + 1 blocks (AAD, CT, lengths), every one a full 16-byte block with the
// 2^128 bit.  Three launches:
//   k_poly1305_prep    one workgroup per slice: the one-time key (one ChaCha20 block, counter 0,
//                      or the caller's), r clamped, the table r^1 .. r^T by doubling in LDS, and
//                      r^CB (CB = blocks per chunk) by squaring.
//   k_poly1305         one workgroup per chunk of P13_CHUNK bytes of one slice's AAD.  Chunks
//                      are cut from the slice's END (the first one is the remainder), so that
//                      every later chunk's partial enters the slice's sum by the one constant
//                      r^CB.  Of the chunk's n blocks lane t of T takes those with index
//                      = n + t (mod T): its last block is always T - t blocks before the end, so
//                      it runs Horner with r^T (acc <- acc r^T + m) and scales by r^(T - t), a
//                      table entry whatever n is.  Loads are 16 B per lane, contiguous across the
//                      wave (non-temporal) when the chunk's base is 16-byte aligned, bytewise
//                      otherwise.  The workgroup adds its lanes' values; the partial is the
//                      chunk's sum with its last block at r^1.
//   k_poly1305_finish  one workgroup per slice: (1) thread 0 folds the chunk partials, h <- h
//                      r^CB + P_c; (2) the CT blocks and (3) the lengths block are one more
//                      sequence absorbed by the same lane-strided Horner, h being added to the
//                      block of index 0 (Poly1305's h <- (h + m) r), so no power of r depends on
//                      the data; (4) thread 0 carries fully, subtracts p when h >= p, adds s with
//                      the carry out of bit 128 dropped.
// No workspace state survives a call and nothing is zeroed: every word read was written earlier
// in the same call.
#include "codec_common.h"
#include "codec_tcc_aead.h"
#include "codec_tcc_blind_keyed.h"

#define P13_CHUNK (256u * 1024u)
#define P13_T 256
#define P13_CB (P13_CHUNK / 16u)           // blocks per chunk = T * 2^P13_CB_SQ
#define P13_CB_SQ 6
#define P13_PW_STRIDE ((P13_T + 1) * 5 + 3)   // words of a slice's table: [0] = r^CB, [e] = r^e, e = 1 .. T
#define P13_M26 0x3FFFFFFu
static_assert(P13_CB == (unsigned)P13_T << P13_CB_SQ, "r^CB is r^T squared P13_CB_SQ times");

// ------------------------------------------------------------------ ChaCha20
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) {
    return __builtin_amdgcn_alignbit(x, x, 32 - n);   // ({x, x} >> (32 - n)): rotate left by n
}
#define CHACHA_QR(a, b, c, d)                \
    a += b; d = rotl32(d ^ a, 16);           \
    c += d; b = rotl32(b ^ c, 12);           \
    a += b; d = rotl32(d ^ a, 8);            \
    c += d; b = rotl32(b ^ c, 7)

__device__ __forceinline__ uint32_t chacha_const(int q) {
    return q == 0 ? 0x61707865u : q == 1 ? 0x3320646Eu : q == 2 ? 0x79622D32u : 0x6B206574u;
}

// the whole block in one lane: x[16] out
__device__ __forceinline__ void chacha_block(const uint32_t* __restrict__ key, uint32_t ctr, uint32_t n0, uint32_t n1,
                                             uint32_t n2, uint32_t* x) {
    uint32_t in[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) in[i] = chacha_const(i);
#pragma unroll
    for (int i = 0; i < 8; ++i) in[4 + i] = key[i];
    in[12] = ctr; in[13] = n0; in[14] = n1; in[15] = n2;
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        CHACHA_QR(x[0], x[4], x[8], x[12]); CHACHA_QR(x[1], x[5], x[9], x[13]);
        CHACHA_QR(x[2], x[6], x[10], x[14]); CHACHA_QR(x[3], x[7], x[11], x[15]);
        CHACHA_QR(x[0], x[5], x[10], x[15]); CHACHA_QR(x[1], x[6], x[11], x[12]);
        CHACHA_QR(x[2], x[7], x[8], x[13]); CHACHA_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += in[i];
}

template <int CTRL> __device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
#define QP_FROM_NEXT1 0x39   // quad_perm [1,2,3,0]: lane q reads lane q + 1 (mod 4)
#define QP_FROM_NEXT2 0x4E   // quad_perm [2,3,0,1]
#define QP_FROM_NEXT3 0x93   // quad_perm [3,0,1,2]: lane q reads lane q + 3 = q - 1

__device__ __forceinline__ uint32_t sel4(int k, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    return k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3;
}

// the block spread over a quad: lane q = lane & 3 gets words 4q .. 4q+3 in o[0..3]
__device__ __forceinline__ void chacha_block_quad(const uint32_t* __restrict__ key, uint32_t ctr, uint32_t n0, uint32_t n1,
                                                  uint32_t n2, int q, uint32_t* o) {
    const uint32_t ia = chacha_const(q), ib = sel4(q, key[0], key[1], key[2], key[3]),
                   ic = sel4(q, key[4], key[5], key[6], key[7]), id = sel4(q, ctr, n0, n1, n2);
    uint32_t a = ia, b = ib, c = ic, d = id;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        CHACHA_QR(a, b, c, d);
        b = quad_perm<QP_FROM_NEXT1>(b); c = quad_perm<QP_FROM_NEXT2>(c); d = quad_perm<QP_FROM_NEXT3>(d);
        CHACHA_QR(a, b, c, d);
        b = quad_perm<QP_FROM_NEXT3>(b); c = quad_perm<QP_FROM_NEXT2>(c); d = quad_perm<QP_FROM_NEXT1>(d);
    }
    a += ia; b += ib; c += ic; d += id;   // lane j: element e is word 4e + j
    // transpose: lane q wants, from lane j, that lane's element q (= word 4q + j).  With k = q - j
    // (mod 4) lane j offers s_k = its element (j + k) % 4, and lane q reads s_k from lane q - k.
    const uint32_t s0 = sel4(q, a, b, c, d), s1 = sel4((q + 1) & 3, a, b, c, d),
                   s2 = sel4((q + 2) & 3, a, b, c, d), s3 = sel4((q + 3) & 3, a, b, c, d);
    const uint32_t r0 = s0, r1 = quad_perm<QP_FROM_NEXT3>(s1), r2 = quad_perm<QP_FROM_NEXT2>(s2),
                   r3 = quad_perm<QP_FROM_NEXT1>(s3);          // r_k = word 4q + (q - k) % 4
#pragma unroll
    for (int m = 0; m < 4; ++m) o[m] = sel4((q - m) & 3, r0, r1, r2, r3);
}

// the bits of word w of a row that lie below bit L of the row
__device__ __forceinline__ u64 mask_word(u64 v, uint32_t w, uint32_t L) {
    const long long rem = (long long)L - 64ll * (long long)w;
    return rem >= 64 ? v : rem <= 0 ? 0ull : v & ((1ull << rem) - 1ull);
}
__device__ __forceinline__ uint32_t row_bits(const int32_t* __restrict__ lengths, u64 b, uint32_t row_words) {
    const long long L = lengths ? (long long)lengths[b] : 0ll;
    return (uint32_t)min(max(L, 0ll), 64ll * (long long)row_words);
}

// VARIANT as above.  RELEASE: tg / tw are compared, ok[] written, and the stores are zero for a slice
// whose tags differ (a mask, not a branch).  NONCES: slice b takes (g, nonce) from n12[b]
// (codec_tcc_blind_keyed.h) instead of (index0 + b, ctx's nonce).
template <int VARIANT, bool RELEASE, bool NONCES>
__global__ __launch_bounds__(256) void k_chacha20_rows(const codec_aead_ctx* __restrict__ ctx, uint32_t index0,
                                                       const uint32_t* __restrict__ n12, const u64* in,
                                                       uint32_t row_words, uint32_t bpr, u64 nitems,
                                                       const int32_t* __restrict__ lengths, u64* out,
                                                       const uint32_t* __restrict__ tg, const uint32_t* __restrict__ tw,
                                                       int32_t* __restrict__ ok) {
    const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 item = VARIANT == 1 ? tid >> 2 : tid;
    if (item >= nitems) return;   // whole quads leave together (block sizes are multiples of 4)
    const int q = (int)(tid & 3);
    const u64 b = item / bpr;
    const uint32_t blk = (uint32_t)(item % bpr);
    const uint32_t L = row_bits(lengths, b, row_words);
    u64 keep = ~0ull;
    if constexpr (RELEASE) {
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) diff |= tg[4 * b + i] ^ tw[4 * b + i];
        keep = diff == 0 ? ~0ull : 0ull;
        if (blk == 0 && (VARIANT == 0 || q == 0)) ok[b] = diff == 0 ? 1 : 0;
    }
    const uint32_t g = NONCES ? n12[3 * b] : index0 + (uint32_t)b;
    const uint32_t n0 = NONCES ? n12[3 * b + 1] : ctx->nonce[0], n1 = NONCES ? n12[3 * b + 2] : ctx->nonce[1];
    const u64* ri = in + b * row_words;
    u64* ro = out + b * row_words;
    if constexpr (VARIANT == 1) {
        uint32_t o[4];
        chacha_block_quad(ctx->key, blk + 1u, g, n0, n1, q, o);
        const uint32_t w0 = blk * 8u + 2u * (uint32_t)q;
        if (w0 < row_words) ro[w0] = mask_word(ri[w0] ^ (((u64)o[1] << 32) | o[0]), w0, L) & keep;
        if (w0 + 1 < row_words) ro[w0 + 1] = mask_word(ri[w0 + 1] ^ (((u64)o[3] << 32) | o[2]), w0 + 1, L) & keep;
    } else {
        uint32_t x[16];
        chacha_block(ctx->key, blk + 1u, g, n0, n1, x);
        u64 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t w = blk * 8u + i;
            v[i] = w < row_words ? ri[w] : 0ull;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t w = blk * 8u + i;
            if (w < row_words) ro[w] = mask_word(v[i] ^ (((u64)x[2 * i + 1] << 32) | x[2 * i]), w, L) & keep;
        }
    }
}

// ------------------------------------------------------------------ Poly1305
struct P13 { uint32_t v[5]; };

// h * r mod p, partially reduced: limbs 0, 2, 3, 4 < 2^26, limb 1 < 2^26 + 2^12 (2^26 + 2^9 for the
// values that occur: limbs of h < 2^28, of r < 2^26 + 2^9).  Inputs: limbs of h < 2^29, of r < 2^27, so that
// 5 r fits 32 bits and the five products of a column 64.
__device__ __forceinline__ P13 p13_mul(const P13& h, const P13& r) {
    const uint32_t s1 = r.v[1] * 5u, s2 = r.v[2] * 5u, s3 = r.v[3] * 5u, s4 = r.v[4] * 5u;
    u64 d0 = (u64)h.v[0] * r.v[0] + (u64)h.v[1] * s4 + (u64)h.v[2] * s3 + (u64)h.v[3] * s2 + (u64)h.v[4] * s1;
    u64 d1 = (u64)h.v[0] * r.v[1] + (u64)h.v[1] * r.v[0] + (u64)h.v[2] * s4 + (u64)h.v[3] * s3 + (u64)h.v[4] * s2;
    u64 d2 = (u64)h.v[0] * r.v[2] + (u64)h.v[1] * r.v[1] + (u64)h.v[2] * r.v[0] + (u64)h.v[3] * s4 + (u64)h.v[4] * s3;
    u64 d3 = (u64)h.v[0] * r.v[3] + (u64)h.v[1] * r.v[2] + (u64)h.v[2] * r.v[1] + (u64)h.v[3] * r.v[0] + (u64)h.v[4] * s4;
    u64 d4 = (u64)h.v[0] * r.v[4] + (u64)h.v[1] * r.v[3] + (u64)h.v[2] * r.v[2] + (u64)h.v[3] * r.v[1] + (u64)h.v[4] * r.v[0];
    P13 o;
    d1 += d0 >> 26; o.v[0] = (uint32_t)d0 & P13_M26;
    d2 += d1 >> 26; o.v[1] = (uint32_t)d1 & P13_M26;
    d3 += d2 >> 26; o.v[2] = (uint32_t)d2 & P13_M26;
    d4 += d3 >> 26; o.v[3] = (uint32_t)d3 & P13_M26;
    o.v[4] = (uint32_t)d4 & P13_M26;
    const u64 t = (u64)o.v[0] + (d4 >> 26) * 5ull;   // 2^130 = 5 (mod p)
    o.v[0] = (uint32_t)t & P13_M26;
    o.v[1] += (uint32_t)(t >> 26);
    return o;
}
__device__ __forceinline__ P13 p13_add(const P13& a, const P13& b) {
    P13 o;
#pragma unroll
    for (int i = 0; i < 5; ++i) o.v[i] = a.v[i] + b.v[i];
    return o;
}
// the four little-endian words of a block as limbs; hibit = 1 << 24 adds the block's 2^128
__device__ __forceinline__ P13 p13_limbs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit) {
    P13 o;
    o.v[0] = w0 & P13_M26;
    o.v[1] = ((w0 >> 26) | (w1 << 6)) & P13_M26;
    o.v[2] = ((w1 >> 20) | (w2 << 12)) & P13_M26;
    o.v[3] = ((w2 >> 14) | (w3 << 18)) & P13_M26;
    o.v[4] = (w3 >> 8) | hibit;
    return o;
}
__device__ __forceinline__ P13 p13_load(const uint32_t* __restrict__ p) {
    P13 o;
#pragma unroll
    for (int i = 0; i < 5; ++i) o.v[i] = p[i];
    return o;
}
// n <= 16 bytes at p as a zero-padded block
__device__ __forceinline__ uint4 p13_gather_bytes(const uint8_t* __restrict__ p, unsigned n) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (unsigned k = 0; k < 16; ++k)
        if (k < n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The workgroup's sum of every lane's value, carried to limbs < 2^26 (the value itself may still
// be >= p), in thread 0.  s_red: 5 * (P13_T / 64) words of 64 bits.
__device__ __forceinline__ P13 p13_wg_sum(const P13& x, u64* s_red) {
    const unsigned t = threadIdx.x;
    u64 l[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        l[i] = x.v[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) l[i] += __shfl_xor(l[i], o, 64);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) s_red[(t >> 6) * 5 + i] = l[i];
    }
    __syncthreads();
    P13 o = {};
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            l[i] = 0;
#pragma unroll
            for (int w = 0; w < P13_T / 64; ++w) l[i] += s_red[w * 5 + i];
        }
        // two passes: after the first, limbs 1..4 < 2^26 and limb 0 < 2^26 + 5 * 2^11; the second
        // leaves every limb < 2^26 (its wrap-around carry is 0 or 1 and meets a small limb 0)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { l[i + 1] += l[i] >> 26; l[i] &= P13_M26; }
            l[0] += (l[4] >> 26) * 5ull;
            l[4] &= P13_M26;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) o.v[i] = (uint32_t)l[i];
    }
    return o;
}

// One workgroup per slice: one-time key, clamped r, power table.  n12 (or NULL): the slices' own
// (g, nonce) in place of (index0 + b, ctx's nonce).
__global__ __launch_bounds__(P13_T) void k_poly1305_prep(const codec_aead_ctx* __restrict__ ctx, uint32_t index0,
                                                         const uint32_t* __restrict__ n12,
                                                         const uint32_t* __restrict__ otk_in,
                                                         uint32_t* __restrict__ ws_s, uint32_t* __restrict__ ws_pw) {
    __shared__ uint32_t s_pw[P13_T + 1][5];
    const unsigned t = threadIdx.x;
    const u64 b = blockIdx.x;
    uint32_t* pw = ws_pw + b * P13_PW_STRIDE;
    if (t == 0) {
        uint32_t k[8];
        if (otk_in) {
#pragma unroll
            for (int i = 0; i < 8; ++i) k[i] = otk_in[8 * b + i];
        } else {
            uint32_t x[16];
            chacha_block(ctx->key, 0u, n12 ? n12[3 * b] : index0 + (uint32_t)b, n12 ? n12[3 * b + 1] : ctx->nonce[0],
                         n12 ? n12[3 * b + 2] : ctx->nonce[1], x);
#pragma unroll
            for (int i = 0; i < 8; ++i) k[i] = x[i];
        }
        const P13 r = p13_limbs(k[0] & 0x0FFFFFFFu, k[1] & 0x0FFFFFFCu, k[2] & 0x0FFFFFFCu, k[3] & 0x0FFFFFFCu, 0u);
#pragma unroll
        for (int i = 0; i < 5; ++i) s_pw[1][i] = r.v[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) ws_s[4 * b + i] = k[4 + i];
    }
    __syncthreads();
    // r^1 .. r^k known: r^(k + j) = r^k r^j for j = 1 .. k (reads <= k, writes > k)
    for (unsigned k = 1; k < P13_T; k <<= 1) {
        if (t >= 1 && t <= k) {
            const P13 x = p13_mul(p13_load(s_pw[k]), p13_load(s_pw[t]));
#pragma unroll
            for (int i = 0; i < 5; ++i) s_pw[k + t][i] = x.v[i];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) pw[(t + 1) * 5 + i] = s_pw[t + 1][i];
    if (t == 0) {
        P13 x = p13_load(s_pw[P13_T]);
        for (int i = 0; i < P13_CB_SQ; ++i) x = p13_mul(x, x);
#pragma unroll
        for (int i = 0; i < 5; ++i) pw[i] = x.v[i];
    }
}

// lane t's Horner over blocks first, first + T, ... < nblk of the chunk at p0; blocks < nfull are
// whole 16 bytes, block nfull (if < nblk) has `tail` bytes
template <bool ALIGNED>
__device__ __forceinline__ P13 p13_lane(const uint8_t* __restrict__ p0, unsigned first, unsigned nblk, unsigned nfull,
                                        unsigned tail, const P13& R) {
    P13 acc = {};
    unsigned i = first;
    if constexpr (ALIGNED) {
        const uint4* vp = reinterpret_cast<const uint4*>(p0);
        for (; i + 3 * P13_T < nfull; i += 4 * P13_T) {
            uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = ldv<true>(vp + i + u * P13_T);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                acc = p13_add(p13_mul(acc, R), p13_limbs(x[u].x, x[u].y, x[u].z, x[u].w, 1u << 24));
        }
        for (; i < nfull; i += P13_T) {
            const uint4 x = ldv<true>(vp + i);
            acc = p13_add(p13_mul(acc, R), p13_limbs(x.x, x.y, x.z, x.w, 1u << 24));
        }
    } else {
        for (; i < nfull; i += P13_T) {
            const uint4 x = p13_gather_bytes(p0 + (size_t)i * 16, 16);
            acc = p13_add(p13_mul(acc, R), p13_limbs(x.x, x.y, x.z, x.w, 1u << 24));
        }
    }
    if (i < nblk) {   // the slice's last, partial block: zero-padded, still a full block
        const uint4 x = p13_gather_bytes(p0 + (size_t)i * 16, tail);
        acc = p13_add(p13_mul(acc, R), p13_limbs(x.x, x.y, x.z, x.w, 1u << 24));
    }
    return acc;
}

__global__ __launch_bounds__(P13_T) void k_poly1305(const uint8_t* __restrict__ aad, u64 n, uint32_t nch,
                                                    const uint32_t* __restrict__ ws_pw, uint32_t* __restrict__ part) {
    __shared__ u64 s_red[5 * (P13_T / 64)];
    const unsigned t = threadIdx.x;
    const u64 b = blockIdx.x / nch;
    const uint32_t c = blockIdx.x % nch;
    const uint32_t* pw = ws_pw + b * P13_PW_STRIDE;
    const u64 na = (n + 15) >> 4;                                  // blocks of the slice
    const u64 nfirst = na - (u64)(nch - 1) * P13_CB;               // of its first chunk (1 .. CB)
    const u64 blk0 = c ? nfirst + (u64)(c - 1) * P13_CB : 0;
    const unsigned nblk = c ? P13_CB : (unsigned)nfirst;
    const uint8_t* p0 = aad + b * n + blk0 * 16;
    const u64 avail = min((u64)nblk * 16, n - blk0 * 16);
    const unsigned nfull = (unsigned)(avail >> 4), tail = (unsigned)(avail & 15);
    const P13 R = p13_load(pw + P13_T * 5);
    const unsigned first = (nblk + t) & (P13_T - 1);
    const P13 acc = ((uintptr_t)p0 & 15) == 0 ? p13_lane<true>(p0, first, nblk, nfull, tail, R)
                                              : p13_lane<false>(p0, first, nblk, nfull, tail, R);
    // the lane's last block lies T - 1 - t blocks before the chunk's last, which stands at r^1
    const P13 sum = p13_wg_sum(p13_mul(acc, p13_load(pw + (P13_T - t) * 5)), s_red);
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) part[(size_t)blockIdx.x * 8 + i] = sum.v[i];
    }
}

__global__ __launch_bounds__(P13_T) void k_poly1305_finish(const uint32_t* __restrict__ part, uint32_t nch, u64 aad_bytes,
                                                           const u64* __restrict__ ct, uint32_t row_words,
                                                           const int32_t* __restrict__ lengths,
                                                           const uint32_t* __restrict__ ws_s,
                                                           const uint32_t* __restrict__ ws_pw, uint32_t* __restrict__ tags) {
    __shared__ u64 s_red[5 * (P13_T / 64)];
    __shared__ uint32_t s_h[5];
    const unsigned t = threadIdx.x;
    const u64 b = blockIdx.x;
    const uint32_t* pw = ws_pw + b * P13_PW_STRIDE;
    if (t == 0) {   // (1) the AAD's sum from its chunks' partials
        P13 h = {};
        const P13 RCB = p13_load(pw);
        for (uint32_t c = 0; c < nch; ++c) h = p13_add(p13_mul(h, RCB), p13_load(part + ((size_t)b * nch + c) * 8));
#pragma unroll
        for (int i = 0; i < 5; ++i) s_h[i] = h.v[i];
    }
    __syncthreads();
    // (2), (3): the CT blocks and the lengths block, h entering with block 0
    const uint32_t L = ct ? row_bits(lengths, b, row_words) : 0u;
    const uint32_t nb = (L + 7) >> 3, nc = (nb + 15) >> 4, nblk = nc + 1;
    const u64* row = ct ? ct + b * row_words : nullptr;   // never read without rows: nc = 0
    const P13 R = p13_load(pw + P13_T * 5);
    P13 acc = {};
    for (uint32_t i = (nblk + t) & (P13_T - 1); i < nblk; i += P13_T) {
        P13 m;
        if (i < nc) {
            const uint32_t w = 2 * i;
            const u64 lo = mask_word(row[w], w, L);
            const u64 hi = w + 1 < row_words ? mask_word(row[w + 1], w + 1, L) : 0ull;
            m = p13_limbs((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 1u << 24);
        } else {
            m = p13_limbs((uint32_t)aad_bytes, (uint32_t)(aad_bytes >> 32), nb, 0u, 1u << 24);
        }
        if (i == 0) m = p13_add(m, p13_load(s_h));
        acc = p13_add(p13_mul(acc, R), m);
    }
    const P13 h = p13_wg_sum(p13_mul(acc, p13_load(pw + (P13_T - t) * 5)), s_red);
    if (t == 0) {   // (4) h < 2^130 with limbs < 2^26: g = h + 5 - 2^130 is h - p; take it when it did not borrow
        uint32_t g[5], c = 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) { g[i] = h.v[i] + c; c = g[i] >> 26; g[i] &= P13_M26; }
        const uint32_t take = 0u - c;   // c = 1: h + 5 >= 2^130, i.e. h >= p
        uint32_t f[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) f[i] = (h.v[i] & ~take) | (g[i] & take);
        const uint32_t w0 = f[0] | (f[1] << 26), w1 = (f[1] >> 6) | (f[2] << 20), w2 = (f[2] >> 12) | (f[3] << 14),
                       w3 = (f[3] >> 18) | (f[4] << 8);
        u64 a = (u64)w0 + ws_s[4 * b];
        tags[4 * b] = (uint32_t)a;
        a = (u64)w1 + ws_s[4 * b + 1] + (a >> 32);
        tags[4 * b + 1] = (uint32_t)a;
        a = (u64)w2 + ws_s[4 * b + 2] + (a >> 32);
        tags[4 * b + 2] = (uint32_t)a;
        a = (u64)w3 + ws_s[4 * b + 3] + (a >> 32);
        tags[4 * b + 3] = (uint32_t)a;
    }
}

// ------------------------------------------------------------------ host
#define AEAD_MAX_ITEMS (1ull << 28)   // (row, block) pairs of one launch: four lanes each stay below 2^31 threads
#define AEAD_MAX_AAD (1ll << 32)      // 2^31 pixels of two bytes

static int aead_index_check(uint32_t index0, int32_t B, const char* who) {
    if (index0 == CODEC_AEAD_STREAM_INDEX && B == 1) return 0;
    if ((u64)index0 + (u64)B > (1ull << 31))
        return set_err(CODEC_EINVAL, "%s: slice indices %u .. %llu are not all < 2^31 (0x80000000 is a stream's, B = 1)", who,
                       index0, (u64)index0 + (u64)B - 1);
    return 0;
}
static int aead_rows_check(int32_t B, int32_t row_words, const char* who) {
    if (B < 1) return set_err(CODEC_EINVAL, "%s: bad batch B=%d", who, B);
    if (row_words < 1 || row_words > CODEC_AEAD_MAX_ROW_WORDS)
        return set_err(CODEC_EINVAL, "%s: row_words=%d outside 1 .. %d", who, row_words, CODEC_AEAD_MAX_ROW_WORDS);
    if ((u64)B * (((u64)row_words + 7) / 8) > AEAD_MAX_ITEMS) return set_err(CODEC_EINVAL, "%s: batch too large", who);
    return 0;
}
// chunks per slice (0 for no AAD); false for arguments beyond the limits
static bool p13_chunks(int32_t B, int64_t aad_bytes, u64* nch) {
    if (B < 1 || aad_bytes < 0 || aad_bytes > AEAD_MAX_AAD) return false;
    *nch = ((u64)aad_bytes + P13_CHUNK - 1) / P13_CHUNK;
    return *nch * (u64)B < (1ull << 22);
}

template <bool RELEASE>
static int chacha_launch(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint32_t* n12, const uint64_t* in,
                         int32_t row_words,
                         const int32_t* lengths, uint64_t* out, const uint32_t* tg, const uint32_t* tw, int32_t* ok,
                         hipStream_t st) {
    const uint32_t bpr = ((uint32_t)row_words + 7u) / 8u;
    const u64 nitems = (u64)B * bpr;
    // layout (A/B, profiles/r14/aead_time.txt: the quad layout is 18 % faster on a 256 MB row): 0 = a lane owns a
    // block, 1 = a quad owns a block
    const long long variant = knob("CODEC_CHACHA_VARIANT", 1);
    const u64 threads = variant == 0 ? nitems : nitems * 4;
    const unsigned wg = threads < 256ull * 256ull ? 64u : 256u;   // small batches: one wave per workgroup, more CUs
    const unsigned grid = (unsigned)((threads + wg - 1) / wg);
    ProfScope prof(st, RELEASE ? CODEC_K_AEAD_RELEASE : CODEC_K_CHACHA20_ROWS);
#define CL(V, N)                                                                                                    \
    hipLaunchKernelGGL((k_chacha20_rows<V, RELEASE, N>), dim3(grid), dim3(wg), 0, st, ctx, index0, n12, (const u64*)in, \
                       (uint32_t)row_words, bpr, nitems, lengths, (u64*)out, tg, tw, ok)
    if (n12) {
        if (variant == 0) CL(0, true);
        else CL(1, true);
    } else {
        if (variant == 0) CL(0, false);
        else CL(1, false);
    }
#undef CL
    LAUNCH_CHECK(RELEASE ? "k_aead_release" : "k_chacha20_rows");
    return 0;
}

static int p13_tags(const char* who, const codec_aead_ctx* ctx, const uint32_t* otk, int32_t B, uint32_t index0,
                    const uint32_t* n12, bool per_slice, const void* aad, int64_t aad_bytes, const uint64_t* ct_rows,
                    int32_t row_words, const int32_t* lengths, uint32_t* tags, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1) return set_err(CODEC_EINVAL, "%s: bad batch B=%d", who, B);
    if (aad_bytes < 0 || aad_bytes > AEAD_MAX_AAD) return set_err(CODEC_EINVAL, "%s: aad_bytes=%lld outside 0 .. 2^32", who, (long long)aad_bytes);
    if ((aad == nullptr) != (aad_bytes == 0)) return set_err(CODEC_EINVAL, "%s: aad is NULL exactly when aad_bytes is 0", who);
    if (row_words == 0) {
        if (ct_rows || lengths) return set_err(CODEC_EINVAL, "%s: row_words=0 goes with ct_rows and lengths NULL", who);
    } else {
        if (int rc = aead_rows_check(B, row_words, who)) return rc;
        if (!ct_rows || !lengths) return set_err(CODEC_EINVAL, "%s: ct_rows and lengths are given together", who);
    }
    u64 nch = 0;
    if (!p13_chunks(B, aad_bytes, &nch)) return set_err(CODEC_EINVAL, "%s: batch too large", who);
    if (!otk && !per_slice) {
        if (int rc = aead_index_check(index0, B, who)) return rc;
    }
    if ((!ctx && !otk) || (per_slice && !n12) || !tags || !workspace) return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    const size_t need = codec_aead_workspace_bytes(B, aad_bytes, row_words);
    if (workspace_bytes < need) return set_err(CODEC_EINVAL, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    uint32_t* ws_s = static_cast<uint32_t*>(workspace);
    uint32_t* ws_pw = ws_s + (size_t)B * 4;
    uint32_t* part = ws_pw + (size_t)B * P13_PW_STRIDE;
    {
        ProfScope prof(st, CODEC_K_POLY1305_PREP);
        hipLaunchKernelGGL(k_poly1305_prep, dim3((unsigned)B), dim3(P13_T), 0, st, ctx, index0, n12, otk, ws_s, ws_pw);
        LAUNCH_CHECK("k_poly1305_prep");
    }
    if (nch) {
        ProfScope prof(st, CODEC_K_POLY1305);
        hipLaunchKernelGGL(k_poly1305, dim3((unsigned)(nch * (u64)B)), dim3(P13_T), 0, st, static_cast<const uint8_t*>(aad),
                           (u64)aad_bytes, (uint32_t)nch, ws_pw, part);
        LAUNCH_CHECK("k_poly1305");
    }
    {
        ProfScope prof(st, CODEC_K_POLY1305_FINISH);
        hipLaunchKernelGGL(k_poly1305_finish, dim3((unsigned)B), dim3(P13_T), 0, st, part, (uint32_t)nch, (u64)aad_bytes,
                           (const u64*)ct_rows, (uint32_t)row_words, lengths, ws_s, ws_pw, tags);
        LAUNCH_CHECK("k_poly1305_finish");
    }
    return 0;
}

extern "C" {

size_t codec_poly1305_chunk_bytes(void) { return P13_CHUNK; }

size_t codec_aead_workspace_bytes(int32_t B, int64_t aad_bytes, int32_t row_words) {
    u64 nch = 0;
    if (!p13_chunks(B, aad_bytes, &nch) || row_words < 0 || row_words > CODEC_AEAD_MAX_ROW_WORDS) return 0;
    return align_up(((size_t)B * (4 + P13_PW_STRIDE) + (size_t)(nch * (u64)B) * 8) * 4, 256);
}

int codec_chacha20_rows(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint64_t* rows_in, int32_t row_words,
                        const int32_t* lengths, uint64_t* rows_out, void* stream) {
    if (int rc = aead_rows_check(B, row_words, "codec_chacha20_rows")) return rc;
    if (int rc = aead_index_check(index0, B, "codec_chacha20_rows")) return rc;
    if (!ctx || !rows_in || !lengths || !rows_out) return set_err(CODEC_EINVAL, "codec_chacha20_rows: NULL pointer argument");
    return chacha_launch<false>(ctx, B, index0, nullptr, rows_in, row_words, lengths, rows_out, nullptr, nullptr, nullptr,
                                as_stream(stream));
}

int codec_poly1305_tags(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const void* aad, int64_t aad_bytes,
                        const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths, uint32_t* tags, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return p13_tags("codec_poly1305_tags", ctx, nullptr, B, index0, nullptr, false, aad, aad_bytes, ct_rows, row_words, lengths, tags,
                    workspace, workspace_bytes, stream);
}

int codec_poly1305_tags_otk(const uint32_t* otk, int32_t B, const void* aad, int64_t aad_bytes, const uint64_t* ct_rows,
                            int32_t row_words, const int32_t* lengths, uint32_t* tags, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!otk) return set_err(CODEC_EINVAL, "codec_poly1305_tags_otk: NULL pointer argument");
    return p13_tags("codec_poly1305_tags_otk", nullptr, otk, B, 0u, nullptr, false, aad, aad_bytes, ct_rows, row_words, lengths, tags,
                    workspace, workspace_bytes, stream);
}

int codec_aead_release(const codec_aead_ctx* ctx, int32_t B, uint32_t index0, const uint32_t* tags_got,
                       const uint32_t* tags_want, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                       uint64_t* pt_rows_out, int32_t* ok, void* stream) {
    if (int rc = aead_rows_check(B, row_words, "codec_aead_release")) return rc;
    if (int rc = aead_index_check(index0, B, "codec_aead_release")) return rc;
    if (!ctx || !ct_rows || !lengths || !pt_rows_out) return set_err(CODEC_EINVAL, "codec_aead_release: NULL pointer argument");
    if (!tags_got || !tags_want || !ok) return set_err(CODEC_EINVAL, "codec_aead_release: NULL tag or ok pointer");
    return chacha_launch<true>(ctx, B, index0, nullptr, ct_rows, row_words, lengths, pt_rows_out, tags_got, tags_want, ok,
                               as_stream(stream));
}

// ---- include/codec_tcc_blind_keyed.h: the same passes with one nonce per slice
int codec_chacha20_rows_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const uint64_t* rows_in,
                          int32_t row_words, const int32_t* lengths, uint64_t* rows_out, void* stream) {
    if (int rc = aead_rows_check(B, row_words, "codec_chacha20_rows_n")) return rc;
    if (!ctx || !nonce12 || !rows_in || !lengths || !rows_out)
        return set_err(CODEC_EINVAL, "codec_chacha20_rows_n: NULL pointer argument");
    return chacha_launch<false>(ctx, B, 0u, nonce12, rows_in, row_words, lengths, rows_out, nullptr, nullptr, nullptr,
                                as_stream(stream));
}

int codec_poly1305_tags_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const void* aad,
                          int64_t aad_bytes, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                          uint32_t* tags, void* workspace, size_t workspace_bytes, void* stream) {
    return p13_tags("codec_poly1305_tags_n", ctx, nullptr, B, 0u, nonce12, true, aad, aad_bytes, ct_rows, row_words, lengths,
                    tags, workspace, workspace_bytes, stream);
}

int codec_aead_release_n(const codec_aead_ctx* ctx, int32_t B, const uint32_t* nonce12, const uint32_t* tags_got,
                         const uint32_t* tags_want, const uint64_t* ct_rows, int32_t row_words, const int32_t* lengths,
                         uint64_t* pt_rows_out, int32_t* ok, void* stream) {
    if (int rc = aead_rows_check(B, row_words, "codec_aead_release_n")) return rc;
    if (!ctx || !nonce12 || !ct_rows || !lengths || !pt_rows_out)
        return set_err(CODEC_EINVAL, "codec_aead_release_n: NULL pointer argument");
    if (!tags_got || !tags_want || !ok) return set_err(CODEC_EINVAL, "codec_aead_release_n: NULL tag or ok pointer");
    return chacha_launch<true>(ctx, B, 0u, nonce12, ct_rows, row_words, lengths, pt_rows_out, tags_got, tags_want, ok,
                               as_stream(stream));
}

}  // extern "C"

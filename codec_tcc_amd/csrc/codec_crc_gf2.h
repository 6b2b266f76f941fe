// codec_crc_gf2.h -- the GF(2) routines of the CRC-32 kernels (codec_crc.hip, codec_tile.hip):
// one routine behind every constant, table and per-lane scaling of both translation units.
//
// A 32-bit register holds a polynomial over GF(2) reflected: bit 31 is x^0, bit 0 is x^31 (the
// arithmetic is set out at the top of codec_crc.hip).  Private to csrc/.
#pragma once
#include "codec_common.h"

#define CRC_POLY 0xEDB88320u
#define CRC_ONE 0x80000000u   // the polynomial 1

// a * b mod P (reflected operands); the one GF(2) routine behind every constant, the combine
// entry and the kernels' per-lane scaling
__host__ __device__ constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (a & (CRC_ONE >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}

// x^n mod P
__host__ __device__ constexpr uint32_t crc_xpow(uint64_t n) {
    uint32_t r = CRC_ONE, s = CRC_ONE >> 1;
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mulmod(r, s);
        s = crc_mulmod(s, s);
    }
    return r;
}

// x^(8 n) mod P for a byte count (8 n may not fit 64 bits: three squarings instead)
static inline uint32_t crc_xpow_bytes(uint64_t n) {
    uint32_t r = crc_xpow(n);
    for (int i = 0; i < 3; ++i) r = crc_mulmod(r, r);
    return r;
}

// [k][b] = (b << 8k) * c, by linearity from the 32 single-bit products
constexpr void crc_fill_mul(uint32_t* tab, uint32_t c) {
    for (int k = 0; k < 4; ++k) {
        uint32_t* t = tab + 256 * k;
        t[0] = 0;
        for (int bit = 0; bit < 8; ++bit) t[1 << bit] = crc_mulmod(1u << (8 * k + bit), c);
        for (int b = 1; b < 256; ++b) t[b] = t[b & (b - 1)] ^ t[b & -b];
    }
}

// u * (the table's constant): tl = table + the lane's copy
template <int R>
__device__ __forceinline__ uint32_t crc_mul_tab(const uint32_t* tl, uint32_t u) {
    return tl[(u & 0xFFu) * R] ^ tl[(256u + ((u >> 8) & 0xFFu)) * R] ^ tl[(512u + ((u >> 16) & 0xFFu)) * R] ^
           tl[(768u + (u >> 24)) * R];
}

// cnt <= 15 bytes at p as the END of a 16-byte vector (leading zero bytes), no indexed registers
__device__ __forceinline__ uint4 crc_gather_bytes(const uint8_t* p, unsigned cnt) {
    u64 lo = 0, hi = 0;
    for (unsigned q = 0; q < cnt; ++q) {
        lo = (lo >> 8) | (hi << 56);
        hi = (hi >> 8) | ((u64)p[q] << 56);
    }
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// the state of the 16 bytes a0..a3 after the states they hold: ((a0 x^32 + a1) x^32 + a2) x^32 + a3
__device__ __forceinline__ uint32_t crc_fold4(const uint32_t* m32, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    uint32_t u = crc_mul_tab<1>(m32, a0) ^ a1;
    u = crc_mul_tab<1>(m32, u) ^ a2;
    return crc_mul_tab<1>(m32, u) ^ a3;
}

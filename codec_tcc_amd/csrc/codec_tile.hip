// codec_tile.hip -- CRC-32 of every 2-D tile of every slice of a batch, and the comparison of two
// such tables (include/codec_tcc_tile.h).  The arithmetic is codec_crc.hip's (state u = M(x) mod P,
// raw CRC = u * x^32, the routines of codec_crc_gf2.h); what differs is the shape of the work:
// many small messages -- a tile's rows, row-major -- instead of one long one per slice.
//
// Vector route (k_tile_crc): every tile row is a whole number of aligned 16-B vectors.  One
// workgroup of 4 waves owns a (slice, tile row) band, fills the tables once (x^(128 * 64) with 8
// copies per entry, x^32 plain: 9 K LDS words) and its waves take the band's tiles in turn.  A
// wave runs k_crc32's scheme with NT = 64 over the tile's nv vectors in message order: lane l
// takes the vectors with index = nv + l (mod 64), so its last one lies 63 - l vectors before the
// tile's end and its scale x^(128 (63 - l)) is a lane constant whatever the tile's height; the
// ragged group is the first.  Four independent states per lane, one fold, one crc_mulmod and a
// wave xor-reduce per tile.  A vector's address follows from (row, column) inside the tile; both
// advance by 64 vectors per step without a division.
//
// Byte route (k_tile_crc_bytes): any width and alignment.  One wave per tile, lane l taking the
// tile rows = h + l (mod 64) bytewise with the x^8 table; a lane's rows are combined with
// x^(8 * 64 * row bytes), the lanes with x^(8 * row bytes)^(63 - l).
//
// The final term 0xFFFFFFFF * x^(8 n) xor 0xFFFFFFFF depends on the tile's byte count n alone,
// which takes four values (interior, last column, last row, corner): the host computes them.
#include "codec_common.h"
#include "codec_crc_gf2.h"
#include "codec_tcc_tile.h"

#define TILE_R 8          // copies per entry of the stride table (k_crc32's default layout)
#define TILE_WAVES 4
#define TILE_MAX_WGS (1u << 20)   // workgroups of a launch: the rest is a grid-stride loop

struct TileConst {
    uint32_t m32[1024];    // [k][b]: (b << 8k) * x^32
    uint32_t ms64[1024];   // ... * x^(128 * 64): the lane stride of one wave
    uint32_t m8[1024];     // ... * x^8 (the byte route reads [0][b] only)
    uint32_t f[64];        // x^(128 j)
};

constexpr TileConst tile_make_const() {
    TileConst c = {};
    crc_fill_mul(c.m32, crc_xpow(32));
    crc_fill_mul(c.ms64, crc_xpow(128ull * 64));
    crc_fill_mul(c.m8, crc_xpow(8));
    const uint32_t x128 = crc_xpow(128);
    c.f[0] = CRC_ONE;
    for (int j = 1; j < 64; ++j) c.f[j] = crc_mulmod(c.f[j - 1], x128);
    return c;
}

__device__ const TileConst d_tile = tile_make_const();

struct TileGeo {
    u64 n;                  // bytes of a slice
    u64 pitch;              // bytes of an image row
    uint32_t H, th, nty, ntx;
    uint32_t twb, ewb;      // bytes of a tile row: every column but the last, the last column
    uint32_t ff[4];         // final term by 2 * (last tile row) + (last tile column)
    uint32_t xr[2], xr64[2];   // byte route: x^(8 row bytes) and its 64th power, by (last tile column)
};

__global__ __launch_bounds__(64 * TILE_WAVES) void k_tile_crc(const uint8_t* __restrict__ img, const TileGeo g,
                                                               const u64 nbands, uint32_t* __restrict__ crc) {
    __shared__ uint32_t s_tab[1024 * TILE_R];
    __shared__ uint32_t s_m32[1024];
    const unsigned t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    for (unsigned i = t; i < 1024; i += 64 * TILE_WAVES) {
        const uint32_t v = d_tile.ms64[i];
#pragma unroll
        for (int r = 0; r < TILE_R; ++r) s_tab[i * TILE_R + r] = v;
        s_m32[i] = d_tile.m32[i];
    }
    __syncthreads();
    const uint32_t* tl = s_tab + (t & (TILE_R - 1));
    const uint32_t fl = d_tile.f[63u - lane];

    for (u64 band = blockIdx.x; band < nbands; band += gridDim.x) {
        const u64 b = band / g.nty;
        const uint32_t ty = (uint32_t)(band % g.nty);
        const uint32_t r0 = ty * g.th, h = min(g.th, g.H - r0);
        const uint8_t* bp = img + b * g.n + (u64)r0 * g.pitch;
        for (uint32_t tx = wv; tx < g.ntx; tx += TILE_WAVES) {
            const bool lastc = tx == g.ntx - 1;
            const uint32_t vpr = (lastc ? g.ewb : g.twb) >> 4;   // vectors of a tile row (>= 1)
            const uint32_t nv = h * vpr;
            const uint8_t* tp = bp + (u64)tx * g.twb;
            // 64 vectors on = qs rows and rs columns on (wave-uniform)
            const uint32_t qs = 64u / vpr, rs = 64u - qs * vpr;
            const u64 dq = (u64)qs * g.pitch + (u64)rs * 16u, wrap = g.pitch - (u64)vpr * 16u;
            uint32_t i = (nv + lane) & 63u;
            uint32_t col = i % vpr;
            u64 off = (u64)(i / vpr) * g.pitch + (u64)col * 16u;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#define TILE_ADV()                                  \
    do {                                            \
        off += dq;                                  \
        col += rs;                                  \
        if (col >= vpr) { col -= vpr; off += wrap; } \
    } while (0)
            if (i < nv) {   // the lane's first vector: nothing to scale yet
                const uint4 v = ldv<true>(reinterpret_cast<const uint4*>(tp + off));
                a0 = v.x; a1 = v.y; a2 = v.z; a3 = v.w;
                i += 64;
                TILE_ADV();
            }
            for (; i + 3 * 64 < nv; i += 4 * 64) {
                uint4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[u] = ldv<true>(reinterpret_cast<const uint4*>(tp + off));
                    TILE_ADV();
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a0 = crc_mul_tab<TILE_R>(tl, a0) ^ x[u].x;
                    a1 = crc_mul_tab<TILE_R>(tl, a1) ^ x[u].y;
                    a2 = crc_mul_tab<TILE_R>(tl, a2) ^ x[u].z;
                    a3 = crc_mul_tab<TILE_R>(tl, a3) ^ x[u].w;
                }
            }
            for (; i < nv; i += 64) {
                const uint4 v = ldv<true>(reinterpret_cast<const uint4*>(tp + off));
                TILE_ADV();
                a0 = crc_mul_tab<TILE_R>(tl, a0) ^ v.x;
                a1 = crc_mul_tab<TILE_R>(tl, a1) ^ v.y;
                a2 = crc_mul_tab<TILE_R>(tl, a2) ^ v.z;
                a3 = crc_mul_tab<TILE_R>(tl, a3) ^ v.w;
            }
#undef TILE_ADV
            // the lane's last vector lies 63 - lane vectors before the tile's end
            uint32_t u = crc_mulmod(crc_fold4(s_m32, a0, a1, a2, a3), fl);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) u ^= __shfl_xor(u, o, 64);
            if (lane == 0) {
                const uint32_t ff = g.ff[(ty == g.nty - 1 ? 2u : 0u) + (lastc ? 1u : 0u)];
                crc[band * g.ntx + tx] = crc_mul_tab<1>(s_m32, u) ^ ff;   // raw CRC = state * x^32
            }
        }
    }
}

// a^k, k < 64
__device__ __forceinline__ uint32_t crc_pow64(uint32_t a, unsigned k) {
    uint32_t r = CRC_ONE;
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        if (k & 1u) r = crc_mulmod(r, a);
        a = crc_mulmod(a, a);
        k >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(64) void k_tile_crc_bytes(const uint8_t* __restrict__ img, const TileGeo g,
                                                        const u64 ntiles, uint32_t* __restrict__ crc) {
    __shared__ uint32_t s_t8[256];
    const unsigned lane = threadIdx.x;
    for (unsigned i = lane; i < 256; i += 64) s_t8[i] = d_tile.m8[i];
    __syncthreads();
    // the lane's last row lies 63 - lane rows above the tile's end
    const uint32_t pw0 = crc_pow64(g.xr[0], 63u - lane), pw1 = crc_pow64(g.xr[1], 63u - lane);
    constexpr uint32_t x32 = crc_xpow(32);

    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t tx = (uint32_t)(tile % g.ntx);
        const u64 band = tile / g.ntx;
        const uint32_t ty = (uint32_t)(band % g.nty);
        const u64 b = band / g.nty;
        const bool lastc = tx == g.ntx - 1;
        const uint32_t wb = lastc ? g.ewb : g.twb;
        const uint32_t x64 = lastc ? g.xr64[1] : g.xr64[0];
        const uint32_t r0 = ty * g.th, h = min(g.th, g.H - r0);
        const uint8_t* tp = img + b * g.n + (u64)r0 * g.pitch + (u64)tx * g.twb;
        uint32_t acc = 0;
        bool first = true;
        for (uint32_t r = (h + lane) & 63u; r < h; r += 64) {
            const uint8_t* p = tp + (u64)r * g.pitch;
            uint32_t u = 0;
            for (uint32_t q = 0; q < wb; ++q) u = (u >> 8) ^ s_t8[u & 0xFFu] ^ ((uint32_t)p[q] << 24);
            acc = first ? u : (crc_mulmod(acc, x64) ^ u);
            first = false;
        }
        uint32_t u = crc_mulmod(acc, lastc ? pw1 : pw0);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) u ^= __shfl_xor(u, o, 64);
        if (lane == 0) {
            const uint32_t ff = g.ff[(ty == g.nty - 1 ? 2u : 0u) + (lastc ? 1u : 0u)];
            crc[tile] = crc_mulmod(u, x32) ^ ff;
        }
    }
}

// one workgroup per slice: wave w takes the bitmap words w, w + 4, ...; plain stores only
__global__ __launch_bounds__(64 * TILE_WAVES) void k_tile_compare(const uint32_t* __restrict__ got,
                                                                   const uint32_t* __restrict__ want, const uint32_t B,
                                                                   const uint32_t nt, u64* __restrict__ bitmap,
                                                                   int32_t* __restrict__ count) {
    __shared__ uint32_t s_cnt[TILE_WAVES];
    const unsigned t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t nw = (nt + 63u) >> 6;
    for (uint32_t b = blockIdx.x; b < B; b += gridDim.x) {
        const uint32_t* gp = got + (u64)b * nt;
        const uint32_t* wp = want + (u64)b * nt;
        uint32_t c = 0;
        for (uint32_t w = wv; w < nw; w += TILE_WAVES) {
            const uint32_t i = w * 64u + lane;
            const bool d = i < nt && gp[i] != wp[i];
            const u64 m = __ballot(d);
            if (lane == 0) bitmap[(u64)b * nw + w] = m;
            c += (uint32_t)__popcll(m);
        }
        if (lane == 0) s_cnt[wv] = c;
        __syncthreads();
        if (t == 0) {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < TILE_WAVES; ++w) s += s_cnt[w];
            count[b] = (int32_t)s;
        }
        __syncthreads();   // s_cnt is reused by the next slice
    }
}

// the checks the entries share: 0 and the grid, or a negative status with its text
static int tile_grid(const char* who, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t* nty, int32_t* ntx) {
    if (H < 1 || W < 1) return set_err(CODEC_EINVAL, "%s: bad shape H=%d W=%d", who, H, W);
    if (th < CODEC_TILE_MIN || th > CODEC_TILE_MAX || tw < CODEC_TILE_MIN || tw > CODEC_TILE_MAX)
        return set_err(CODEC_EINVAL, "%s: tile size (%d, %d) outside %d..%d", who, th, tw, CODEC_TILE_MIN, CODEC_TILE_MAX);
    if ((long long)H * W > (1LL << 31)) return set_err(CODEC_EINVAL, "%s: slice too large", who);
    *nty = (int32_t)(((long long)H + th - 1) / th);
    *ntx = (int32_t)(((long long)W + tw - 1) / tw);
    return 0;
}

static int tile_args(const char* who, int32_t B, int32_t H, int32_t W, int32_t bytes, int32_t th, int32_t tw,
                     const void* images, int32_t* nty, int32_t* ntx) {
    if (B < 1) return set_err(CODEC_EINVAL, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    if (bytes != 1 && bytes != 2) return set_err(CODEC_EINVAL, "%s: bytes must be 1 or 2", who);
    const int rc = tile_grid(who, H, W, th, tw, nty, ntx);
    if (rc) return rc;
    if ((long long)B * *nty * (long long)*ntx >= (1LL << 31))
        return set_err(CODEC_EINVAL, "%s: batch too large (B * nty * ntx >= 2^31)", who);
    if (!images) return set_err(CODEC_EINVAL, "%s: NULL pointer argument", who);
    return 0;
}

static bool tile_vector_route(int32_t W, int32_t bytes, int32_t tw, const void* images) {
    return ((long long)tw * bytes) % 16 == 0 && ((long long)W * bytes) % 16 == 0 && ((uintptr_t)images & 15u) == 0;
}

extern "C" {

int codec_crc32_tiles_grid(int32_t H, int32_t W, int32_t th, int32_t tw, int32_t* nty, int32_t* ntx) {
    if (!nty || !ntx) return set_err(CODEC_EINVAL, "codec_crc32_tiles_grid: NULL pointer argument");
    return tile_grid("codec_crc32_tiles_grid", H, W, th, tw, nty, ntx);
}

int codec_crc32_tiles_route(int32_t B, int32_t H, int32_t W, int32_t bytes, int32_t th, int32_t tw,
                            const void* images) {
    int32_t nty = 0, ntx = 0;
    const int rc = tile_args("codec_crc32_tiles_route", B, H, W, bytes, th, tw, images, &nty, &ntx);
    if (rc) return rc;
    return tile_vector_route(W, bytes, tw, images) ? CODEC_TILE_ROUTE_VECTOR : CODEC_TILE_ROUTE_BYTES;
}

int codec_crc32_tiles(int32_t B, int32_t H, int32_t W, int32_t bytes, int32_t th, int32_t tw, const void* images,
                      uint32_t* crc, void* stream) {
    int32_t nty = 0, ntx = 0;
    const int rc = tile_args("codec_crc32_tiles", B, H, W, bytes, th, tw, images, &nty, &ntx);
    if (rc) return rc;
    if (!crc) return set_err(CODEC_EINVAL, "codec_crc32_tiles: NULL pointer argument");
    TileGeo g = {};
    g.pitch = (u64)W * (u64)bytes;
    g.n = (u64)H * g.pitch;
    g.H = (uint32_t)H;
    g.th = (uint32_t)th;
    g.nty = (uint32_t)nty;
    g.ntx = (uint32_t)ntx;
    g.twb = (uint32_t)(tw * bytes);
    g.ewb = (uint32_t)(((long long)W - (long long)(ntx - 1) * tw) * bytes);
    const u64 hh[2] = {(u64)(nty > 1 ? th : H), (u64)((long long)H - (long long)(nty - 1) * th)};
    const u64 wb[2] = {ntx > 1 ? g.twb : g.ewb, g.ewb};
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c)
            g.ff[2 * r + c] = crc_mulmod(0xFFFFFFFFu, crc_xpow_bytes(hh[r] * wb[c])) ^ 0xFFFFFFFFu;
    for (int c = 0; c < 2; ++c) {
        g.xr[c] = crc_xpow_bytes(wb[c]);
        g.xr64[c] = crc_xpow_bytes(64 * wb[c]);
    }
    hipStream_t st = as_stream(stream);
    const uint8_t* img = static_cast<const uint8_t*>(images);
    const u64 nbands = (u64)B * (u64)nty, ntiles = nbands * (u64)ntx;
    if (tile_vector_route(W, bytes, tw, images)) {
        ProfScope prof(st, CODEC_K_TILE_CRC);
        const unsigned wgs = (unsigned)(nbands < TILE_MAX_WGS ? nbands : TILE_MAX_WGS);
        hipLaunchKernelGGL(k_tile_crc, dim3(wgs), dim3(64 * TILE_WAVES), 0, st, img, g, nbands, crc);
        LAUNCH_CHECK("k_tile_crc");
    } else {
        ProfScope prof(st, CODEC_K_TILE_CRC_BYTES);
        const unsigned wgs = (unsigned)(ntiles < TILE_MAX_WGS ? ntiles : TILE_MAX_WGS);
        hipLaunchKernelGGL(k_tile_crc_bytes, dim3(wgs), dim3(64), 0, st, img, g, ntiles, crc);
        LAUNCH_CHECK("k_tile_crc_bytes");
    }
    return 0;
}

int codec_crc32_tiles_compare(int32_t B, int32_t nt, const uint32_t* got, const uint32_t* want, uint64_t* bitmap,
                              int32_t* count, void* stream) {
    if (B < 1 || nt < 1) return set_err(CODEC_EINVAL, "codec_crc32_tiles_compare: bad shape B=%d nt=%d", B, nt);
    if ((long long)B * nt >= (1LL << 31)) return set_err(CODEC_EINVAL, "codec_crc32_tiles_compare: batch too large");
    if (!got || !want || !bitmap || !count)
        return set_err(CODEC_EINVAL, "codec_crc32_tiles_compare: NULL pointer argument");
    hipStream_t st = as_stream(stream);
    ProfScope prof(st, CODEC_K_TILE_COMPARE);
    const unsigned wgs = (unsigned)((u64)B < TILE_MAX_WGS ? (u64)B : TILE_MAX_WGS);
    hipLaunchKernelGGL(k_tile_compare, dim3(wgs), dim3(64 * TILE_WAVES), 0, st, got, want, (uint32_t)B, (uint32_t)nt,
                       reinterpret_cast<u64*>(bitmap), count);
    LAUNCH_CHECK("k_tile_compare");
    return 0;
}

}  // extern "C"

// codec_crc.hip -- CRC-32 (zlib's: reflected 0xEDB88320, init and final xor 0xFFFFFFFF) of
// every slice of a batch in one read-only streaming pass (include/codec_tcc_crc.h).
//
// Arithmetic.  A 32-bit register holds a polynomial over GF(2) reflected: bit 31 is x^0, bit 0
// is x^31.  A little-endian 32-bit load of four message bytes is then the polynomial of those
// 32 message bits as it stands.  Without init and final xor the CRC is linear: the "raw" CRC of
// a message M of n bits is M(x) * x^32 mod P.  The kernel works on the state u = M(x) mod P
// (the raw CRC is u * x^32): appending a word w after a gap that makes the lane's stride S words is
//     u <- u * x^(32 S) mod P  xor  w
// and the multiply by the constant x^(32 S) is four 256-entry table lookups (one per byte of
// u), tables in LDS.
//
// Launch 1 (k_crc32): one workgroup of NT threads per chunk of CRC_CHUNK bytes of one slice.
// Bytes before the first 16-B boundary and after the last one are gathered bytewise into a vector
// with leading zero bytes (leading zeros do not change a raw CRC); the head vector counts as vector
// 0.  Of the chunk's nv vectors thread t takes those with index = nv + t (mod NT), so its last
// one is always NT - 1 - t vectors before the end and its scale x^(128 (NT - 1 - t)) is a constant
// of the lane (table f), whatever nv is.  A thread keeps one state per dword of the vector (four
// independent lookup chains), folds them with the x^32 table at the end, scales by its constant
// (one shift-and-xor multiply in the ALU), and the workgroup xor-reduces.  Thread 0 appends the
// tail bytes and writes the chunk's raw CRC.
// Launch 2 (k_crc32_combine): one thread per slice folds the chunk partials,
//     r <- r * x^(8 len_c) xor part_c,   crc = r xor 0xFFFFFFFF * x^(8 n) xor 0xFFFFFFFF.
//
// Table layout (template R): each table entry is stored R times, lane l reading copy l mod R, so
// with R = 32 every lane of a ds_read_b32 group has a bank of its own, with R = 8 the 32 lanes
// spread over 4 x 8 banks, R = 1 is the plain 4 KiB table.  A/B: profiles/r08/crc_time.txt.
#include "codec_common.h"
#include "codec_crc_gf2.h"
#include "codec_tcc_crc.h"

#define CRC_CHUNK (256u * 1024u)

struct CrcConst {
    uint32_t m32[1024];      // [k][b]: (b << 8k) * x^32
    uint32_t ms256[1024];    // ... * x^(128 * 256): the lane stride of 256 threads
    uint32_t ms1024[1024];   // ... * x^(128 * 1024)
    uint32_t f[1024];        // x^(128 j)
    uint32_t g[16];          // x^(8 j)
};

constexpr CrcConst crc_make_const() {
    CrcConst c = {};
    crc_fill_mul(c.m32, crc_xpow(32));
    crc_fill_mul(c.ms256, crc_xpow(128ull * 256));
    crc_fill_mul(c.ms1024, crc_xpow(128ull * 1024));
    const uint32_t x128 = crc_xpow(128), x8 = crc_xpow(8);
    c.f[0] = CRC_ONE;
    for (int j = 1; j < 1024; ++j) c.f[j] = crc_mulmod(c.f[j - 1], x128);
    c.g[0] = CRC_ONE;
    for (int j = 1; j < 16; ++j) c.g[j] = crc_mulmod(c.g[j - 1], x8);
    return c;
}

__device__ const CrcConst d_crc = crc_make_const();

template <int NT, int R>
__global__ __launch_bounds__(NT) void k_crc32(const uint8_t* __restrict__ img, u64 n, uint32_t nch,
                                              uint32_t* __restrict__ part) {
    __shared__ uint32_t s_tab[1024 * R];
    __shared__ uint32_t s_m32[1024];
    __shared__ uint32_t s_red[NT / 64];
    const unsigned t = threadIdx.x;
    const uint32_t* gs = NT == 256 ? d_crc.ms256 : d_crc.ms1024;
    for (unsigned i = t; i < 1024; i += NT) {
        const uint32_t v = gs[i];
#pragma unroll
        for (int r = 0; r < R; ++r) s_tab[i * R + r] = v;
        s_m32[i] = d_crc.m32[i];
    }
    __syncthreads();
    const uint32_t* tl = s_tab + (t & (R - 1));

    const u64 b = blockIdx.x / nch;
    const uint32_t c = blockIdx.x % nch;
    const u64 c0 = (u64)c * CRC_CHUNK;
    const uint8_t* p0 = img + b * n + c0;
    const unsigned len = (unsigned)min((u64)CRC_CHUNK, n - c0);
    const unsigned h = min(len, (unsigned)((16u - (unsigned)((uintptr_t)p0 & 15u)) & 15u));
    const uint4* vp = reinterpret_cast<const uint4*>(p0 + h);
    const unsigned nv = (len - h) >> 4, tail = (len - h) & 15u;
    const unsigned hv = h ? 1u : 0u;
    const unsigned nvp = nv + hv;   // vector 0 is the gathered head when there is one

    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    unsigned i = (nvp + t) & (NT - 1);
    if (i < nvp) {   // the thread's first vector: nothing to scale yet
        const uint4 v = (hv && i == 0) ? crc_gather_bytes(p0, h) : ldv<true>(vp + (i - hv));
        a0 = v.x; a1 = v.y; a2 = v.z; a3 = v.w;
        i += NT;
    }
    vp -= hv;   // vp[i] is vector i from here on (i >= NT > 0: never the head)
    for (; i + 3 * NT < nvp; i += 4 * NT) {
        uint4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = ldv<true>(vp + i + u * NT);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a0 = crc_mul_tab<R>(tl, a0) ^ x[u].x;
            a1 = crc_mul_tab<R>(tl, a1) ^ x[u].y;
            a2 = crc_mul_tab<R>(tl, a2) ^ x[u].z;
            a3 = crc_mul_tab<R>(tl, a3) ^ x[u].w;
        }
    }
    for (; i < nvp; i += NT) {
        const uint4 v = ldv<true>(vp + i);
        a0 = crc_mul_tab<R>(tl, a0) ^ v.x;
        a1 = crc_mul_tab<R>(tl, a1) ^ v.y;
        a2 = crc_mul_tab<R>(tl, a2) ^ v.z;
        a3 = crc_mul_tab<R>(tl, a3) ^ v.w;
    }
    // the thread's last vector lies NT - 1 - t vectors before the end of the vector region
    uint32_t u = crc_mulmod(crc_fold4(s_m32, a0, a1, a2, a3), d_crc.f[NT - 1 - t]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) u ^= __shfl_xor(u, o, 64);
    if ((t & 63) == 0) s_red[t >> 6] = u;
    __syncthreads();
    if (t == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) s ^= s_red[w];
        if (tail) {
            const uint4 v = crc_gather_bytes(p0 + h + (size_t)nv * 16, tail);
            s = crc_mulmod(s, d_crc.g[tail]) ^ crc_fold4(s_m32, v.x, v.y, v.z, v.w);
        }
        part[blockIdx.x] = crc_mul_tab<1>(s_m32, s);   // raw CRC of the chunk = state * x^32
    }
}

__global__ __launch_bounds__(256) void k_crc32_combine(const uint32_t* __restrict__ part, int B, uint32_t nch,
                                                       uint32_t xchunk, uint32_t xlast, uint32_t ffterm,
                                                       uint32_t* __restrict__ crc) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const uint32_t* p = part + (size_t)b * nch;
    uint32_t r = 0;
    for (uint32_t c = 0; c + 1 < nch; ++c) r = crc_mulmod(r, xchunk) ^ p[c];
    r = crc_mulmod(r, xlast) ^ p[nch - 1];
    crc[b] = r ^ ffterm;
}

// chunks per slice, or 0 for bad arguments (the checks the entries share)
static u64 crc_chunks(int32_t B, int32_t H, int32_t W, int32_t bytes, u64* n_out) {
    if (B < 1 || H < 1 || W < 1 || (bytes != 1 && bytes != 2)) return 0;
    const u64 npx = (u64)H * (u64)W;
    if (npx > (1ull << 31)) return 0;
    const u64 n = npx * (u64)bytes;
    const u64 nch = (n + CRC_CHUNK - 1) / CRC_CHUNK;
    if (nch * (u64)B >= (1ull << 22)) return 0;   // workgroups x 1024 threads stay below 2^32
    if (n_out) *n_out = n;
    return nch;
}

extern "C" {

size_t codec_crc32_chunk_bytes(void) { return CRC_CHUNK; }

size_t codec_crc32_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t bytes) {
    const u64 nch = crc_chunks(B, H, W, bytes, nullptr);
    return nch ? align_up((size_t)(nch * (u64)B * 4), 256) : 0;
}

int codec_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t* out) {
    if (!out) return set_err(CODEC_EINVAL, "codec_crc32_combine: NULL pointer argument");
    *out = crc_mulmod(crc_a, crc_xpow_bytes(len_b)) ^ crc_b;
    return 0;
}

int codec_crc32_slices(int32_t B, int32_t H, int32_t W, int32_t bytes, const void* images, uint32_t* crc,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 1 || H < 1 || W < 1) return set_err(CODEC_EINVAL, "codec_crc32_slices: bad shape B=%d H=%d W=%d", B, H, W);
    if (bytes != 1 && bytes != 2) return set_err(CODEC_EINVAL, "codec_crc32_slices: bytes must be 1 or 2");
    if (!images || !crc || !workspace) return set_err(CODEC_EINVAL, "codec_crc32_slices: NULL pointer argument");
    if ((long long)H * W > (1LL << 31)) return set_err(CODEC_EINVAL, "codec_crc32_slices: slice too large");
    u64 n = 0;
    const u64 nch = crc_chunks(B, H, W, bytes, &n);
    if (!nch) return set_err(CODEC_EINVAL, "codec_crc32_slices: batch too large");
    if (workspace_bytes < codec_crc32_workspace_bytes(B, H, W, bytes))
        return set_err(CODEC_EINVAL, "codec_crc32_slices: workspace too small (%zu < %zu)", workspace_bytes,
                       codec_crc32_workspace_bytes(B, H, W, bytes));
    hipStream_t st = as_stream(stream);
    uint32_t* part = static_cast<uint32_t*>(workspace);
    const uint8_t* img = static_cast<const uint8_t*>(images);
    const unsigned wgs = (unsigned)(nch * (u64)B);
    // table layout / workgroup size (A/B, profiles/r08/crc_time.txt): 0 = plain table, 256 threads;
    // 1 = 8 copies, 256 threads; 2 = 32 copies (one per bank), 1024 threads; 3 = plain, 1024 threads
    const long long variant = knob("CODEC_CRC_VARIANT", 1);
    {
        ProfScope prof(st, CODEC_K_CRC32);
#define CL(NT, R) hipLaunchKernelGGL((k_crc32<NT, R>), dim3(wgs), dim3(NT), 0, st, img, n, (uint32_t)nch, part)
        if (variant == 0) CL(256, 1);
        else if (variant == 2) CL(1024, 32);
        else if (variant == 3) CL(1024, 1);
        else CL(256, 8);
#undef CL
        LAUNCH_CHECK("k_crc32");
    }
    const u64 last = n - (nch - 1) * CRC_CHUNK;
    const uint32_t ffterm = crc_mulmod(0xFFFFFFFFu, crc_xpow_bytes(n)) ^ 0xFFFFFFFFu;
    {
        ProfScope prof(st, CODEC_K_CRC32_COMBINE);
        hipLaunchKernelGGL(k_crc32_combine, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, part, B, (uint32_t)nch,
                           crc_xpow_bytes(CRC_CHUNK), crc_xpow_bytes(last), ffterm, crc);
        LAUNCH_CHECK("k_crc32_combine");
    }
    return 0;
}

}  // extern "C"

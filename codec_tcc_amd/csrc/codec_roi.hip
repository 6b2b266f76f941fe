// codec_roi.hip -- codec_roi_bbox (include/codec_tcc_roi.h): per slice, the bounding rectangle
// of the pixels above a level -- a segmentation mask (level 0) or a cover thresholded against
// its background.  The ROI embed / extract kernels are the GATE = true instantiations of
// codec_pee.hip; the table pass with rectangles is codec_gate.hip's.
//
// Three launches on one stream, no memset and no workspace (capturable):
//   k_roi_init    roi_out[b] = (INT_MAX, INT_MAX, -1, -1): the accumulator (ymin, xmin, ymax, xmax)
//   k_roi_bbox    one read-only streaming pass, grid (regions, B), 256 threads.  A workgroup
//                 takes a contiguous span of the slice (RB_VEC_PER_WG 16-byte vectors, or
//                 RB_PX_PER_WG pixels on the scalar route), each lane folds its pixels into four
//                 registers, the wave reduces them with shuffles (min / max), the four waves
//                 meet in LDS and ONE lane issues the workgroup's four atomics -- none at all
//                 when the span holds no pixel above the level.
//   k_roi_finish  half-open, grown by the margin, clamped; no pixel: (0, 0, 0, 0)
// VEC (the image 16-byte aligned and a row a whole number of vectors, so every slice and every
// row starts on a vector and a vector never spans two rows): the span's first row and column
// come from one uniform division per workgroup, a lane's from a 32-bit one per vector.  Odd
// widths and offset views take the scalar route (one pixel per lane per step).
#include "codec_common.h"
#include "codec_tcc_roi.h"

#include <limits.h>

#define RB_VEC_PER_WG 4096    // 64 KB of a slice per workgroup: 4 steps of 4 vectors per lane
#define RB_PX_PER_WG 16384

struct RoiBox {
    int ymin, xmin, ymax, xmax;
    __device__ __forceinline__ void add(int y, int xlo, int xhi) {
        ymin = min(ymin, y); ymax = max(ymax, y);
        xmin = min(xmin, xlo); xmax = max(xmax, xhi);
    }
};

// bit e set = pixel e of the vector is above the level (8 pixels of uint16_t, 16 of uint8_t)
__device__ __forceinline__ uint32_t rb_mask(const uint4& v, uint32_t level, uint16_t) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m |= ((w[e] & 0xFFFFu) > level ? 1u : 0u) << (2 * e);
        m |= ((w[e] >> 16) > level ? 1u : 0u) << (2 * e + 1);
    }
    return m;
}
__device__ __forceinline__ uint32_t rb_mask(const uint4& v, uint32_t level, uint8_t) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) m |= (((w[e] >> (8 * q)) & 0xFFu) > level ? 1u : 0u) << (4 * e + q);
    return m;
}

__global__ __launch_bounds__(256) void k_roi_init(int32_t* __restrict__ acc, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        acc[4 * b] = INT_MAX; acc[4 * b + 1] = INT_MAX; acc[4 * b + 2] = -1; acc[4 * b + 3] = -1;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_roi_bbox(const T* __restrict__ img, int H, int W, uint32_t level,
                                                  int32_t* __restrict__ acc) {
    __shared__ int sh[4][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const size_t npx = (size_t)H * W;
    const T* src = img + (size_t)b * npx;
    RoiBox bx = {INT_MAX, INT_MAX, -1, -1};
    if constexpr (VEC) {
        constexpr int VL = 16 / (int)sizeof(T);              // pixels per vector
        const uint32_t VR = (uint32_t)W / VL;                // vectors per row (W % VL == 0)
        const uint32_t nvec = (uint32_t)H * VR;              // < 2^32: H, W <= 65535
        const uint32_t v0 = (uint32_t)blockIdx.x * RB_VEC_PER_WG;
        const uint32_t n = min((uint32_t)RB_VEC_PER_WG, nvec - v0);   // v0 < nvec by the grid
        const uint32_t row0 = v0 / VR, c0 = v0 - row0 * VR;  // uniform
        const uint4* vp = reinterpret_cast<const uint4*>(src) + v0;
        constexpr int U = 4;
        for (uint32_t t = tid; t < n; t += 256 * U) {
            uint4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const uint32_t tk = min(t + 256u * k, n - 1u);   // clamped: a valid address (counted twice, harmless)
                v[k] = ldv<true>(vp + tk);
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const uint32_t tk = min(t + 256u * k, n - 1u);
                const uint32_t m = rb_mask(v[k], level, T{});
                if (m) {
                    const uint32_t cv = c0 + tk;             // < VR + 4096
                    const uint32_t dr = cv / VR, col = (cv - dr * VR) * VL;
                    bx.add((int)(row0 + dr), (int)col + __ffs((int)m) - 1, (int)col + 31 - __clz((int)m));
                }
            }
        }
    } else {
        const size_t e0 = (size_t)blockIdx.x * RB_PX_PER_WG;
        const uint32_t n = (uint32_t)min((size_t)RB_PX_PER_WG, npx - e0);    // e0 < npx by the grid
        const uint32_t row0 = (uint32_t)(e0 / (size_t)W), c0 = (uint32_t)(e0 - (size_t)row0 * W);   // uniform
        for (uint32_t t = tid; t < n; t += 256) {
            if ((uint32_t)src[e0 + t] > level) {
                const uint32_t cv = c0 + t;                  // < W + 16384
                const uint32_t dr = cv / (uint32_t)W, col = cv - dr * (uint32_t)W;
                bx.add((int)(row0 + dr), (int)col, (int)col);
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        bx.ymin = min(bx.ymin, __shfl_xor(bx.ymin, o, 64));
        bx.xmin = min(bx.xmin, __shfl_xor(bx.xmin, o, 64));
        bx.ymax = max(bx.ymax, __shfl_xor(bx.ymax, o, 64));
        bx.xmax = max(bx.xmax, __shfl_xor(bx.xmax, o, 64));
    }
    if ((tid & 63) == 0) {
        sh[tid >> 6][0] = bx.ymin; sh[tid >> 6][1] = bx.xmin; sh[tid >> 6][2] = bx.ymax; sh[tid >> 6][3] = bx.xmax;
    }
    __syncthreads();
    if (tid == 0) {
        const int ymin = min(min(sh[0][0], sh[1][0]), min(sh[2][0], sh[3][0]));
        const int xmin = min(min(sh[0][1], sh[1][1]), min(sh[2][1], sh[3][1]));
        const int ymax = max(max(sh[0][2], sh[1][2]), max(sh[2][2], sh[3][2]));
        const int xmax = max(max(sh[0][3], sh[1][3]), max(sh[2][3], sh[3][3]));
        if (ymax >= 0) {   // one set of atomics per workgroup, none for an empty span
            atomicMin(&acc[4 * b], ymin); atomicMin(&acc[4 * b + 1], xmin);
            atomicMax(&acc[4 * b + 2], ymax); atomicMax(&acc[4 * b + 3], xmax);
        }
    }
}

__global__ __launch_bounds__(256) void k_roi_finish(int32_t* __restrict__ acc, int B, int H, int W, int margin) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int ymin = acc[4 * b], xmin = acc[4 * b + 1], ymax = acc[4 * b + 2], xmax = acc[4 * b + 3];
    const bool any = ymax >= 0;
    acc[4 * b] = any ? max(ymin - margin, 0) : 0;
    acc[4 * b + 1] = any ? max(xmin - margin, 0) : 0;
    acc[4 * b + 2] = any ? min(ymax + 1 + margin, H) : 0;
    acc[4 * b + 3] = any ? min(xmax + 1 + margin, W) : 0;
}

extern "C" {

int codec_roi_bbox(const codec_pee_params* P, const void* image, int32_t level, int32_t margin, int32_t* roi_out,
                   void* stream) {
    if (!P) return set_err(CODEC_EINVAL, "codec_roi_bbox: params is NULL");
    if (!codec_pee_workspace_bytes(P)) return CODEC_EINVAL;   // checks P and sets the text
    if (int rc = pee_roi_dim_check(P, "codec_roi_bbox")) return rc;
    if (!image || !roi_out) return set_err(CODEC_EINVAL, "codec_roi_bbox: NULL pointer argument");
    if (level < 0 || level > 65535) return set_err(CODEC_EINVAL, "codec_roi_bbox: level must be in 0..65535");
    if (margin < 0 || margin > 65535) return set_err(CODEC_EINVAL, "codec_roi_bbox: margin must be in 0..65535");
    hipStream_t st = as_stream(stream);
    const unsigned gb = (unsigned)((P->B + 255) / 256);
    hipLaunchKernelGGL(k_roi_init, dim3(gb), dim3(256), 0, st, roi_out, P->B);
    LAUNCH_CHECK("k_roi_init");
    {
        ProfScope prof(st, CODEC_K_ROI_BBOX);
        const int vl = 16 / P->bytes;
        const bool vec = (P->W % vl) == 0 && ((uintptr_t)image % 16) == 0;
        const long long npx = (long long)P->H * P->W;
        const long long units = vec ? (npx / vl + RB_VEC_PER_WG - 1) / RB_VEC_PER_WG : (npx + RB_PX_PER_WG - 1) / RB_PX_PER_WG;
        dim3 grid((unsigned)units, (unsigned)P->B);   // >= 1: H, W >= 1
        pee_pixel(P->bytes, [&](auto px) {
            const auto* img = static_cast<const decltype(px)*>(image);
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, img, P->H, P->W, (uint32_t)level, roi_out); };
            pee_flag(vec, [&](auto v) { go(k_roi_bbox<decltype(px), v()>); });
        });
        LAUNCH_CHECK("k_roi_bbox");
    }
    hipLaunchKernelGGL(k_roi_finish, dim3(gb), dim3(256), 0, st, roi_out, P->B, P->H, P->W, (int)margin);
    LAUNCH_CHECK("k_roi_finish");
    return 0;
}

}  // extern "C"

// Host sanitizer check of the argument validation of include/codec_tcc_vol.h's entries, as
// abi_args_crc.cpp is for codec_tcc_crc.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status (0 for the size query) with an error text and no device operation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_vol.h"

#include "abi_expect.h"

static codec_pee_params good() {
    codec_pee_params P;
    memset(&P, 0, sizeof(P));
    P.B = 5; P.H = 64; P.W = 96; P.bytes = 2; P.T = 1; P.maxval = 4095;
    P.payload_words = 4; P.lm_words = 24;   // (64 / 2) * (96 / 2) = 1536 candidates
    return P;
}

// the parameter sets every entry must refuse
static int bad_params(codec_pee_params* out) {
    int k = 0;
    codec_pee_params P;
    P = good(); P.B = 0; out[k++] = P;
    P = good(); P.B = -3; out[k++] = P;
    P = good(); P.B = INT32_MIN; out[k++] = P;
    P = good(); P.H = 0; out[k++] = P;
    P = good(); P.W = -1; out[k++] = P;
    P = good(); P.H = 65536; P.W = 65536; P.lm_words = 1 << 24; out[k++] = P;      // H * W past 2^31
    P = good(); P.bytes = 0; out[k++] = P;
    P = good(); P.bytes = 4; out[k++] = P;
    P = good(); P.T = 0; out[k++] = P;
    P = good(); P.maxval = 0; out[k++] = P;
    P = good(); P.maxval = 65536; out[k++] = P;
    P = good(); P.bytes = 1; P.maxval = 256; out[k++] = P;
    P = good(); P.payload_words = 0; out[k++] = P;
    P = good(); P.payload_words = -1; out[k++] = P;
    P = good(); P.lm_words = 0; out[k++] = P;
    P = good(); P.lm_words = 23; out[k++] = P;                                     // 1472 < 1536 candidates
    P = good(); P.B = 2048; P.H = 2048; P.W = 2048; P.lm_words = 16384; out[k++] = P;   // 2^31 candidates
    P = good(); P.B = INT32_MAX; out[k++] = P;
    P = good(); P.B = 1 << 20; P.H = 2; P.W = 2; P.lm_words = 1; P.payload_words = 1 << 11; out[k++] = P;   // B * payload_words = 2^31
    P = good(); P.payload_words = INT32_MAX; out[k++] = P;
    return k;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    uint64_t* u64p = reinterpret_cast<uint64_t*>(buf);
    codec_pee_meta* meta = reinterpret_cast<codec_pee_meta*>(buf);
    codec_pee_volume_info* info = reinterpret_cast<codec_pee_volume_info*>(buf);
    const size_t big = (size_t)1 << 40;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }
    if (sizeof(codec_pee_volume_info) != 32) { fprintf(stderr, "FAIL info size\n"); ++g_fail; }

    codec_pee_params G = good();
    const size_t pws = codec_pee_workspace_bytes(&G);
    const size_t vws = codec_pee_volume_workspace_bytes(&G, 16);
    const size_t vws1 = codec_pee_volume_workspace_bytes(&G, 1);
    if (!pws) { fprintf(stderr, "FAIL codec_pee_workspace_bytes of good arguments\n"); ++g_fail; }
    if (vws < 5 * 16 * 4 + 5 * 4 * 8 + 6 * 4 || vws1 < 5 * 4 * 8 + 6 * 4 || vws1 > vws) {
        fprintf(stderr, "FAIL volume workspace_bytes of good arguments: %zu / %zu\n", vws, vws1);
        ++g_fail;
    }

    // ---- the size query
    EXPECT_EQ(codec_pee_volume_workspace_bytes(nullptr, 16), 0);
    EXPECT_EQ(codec_pee_volume_workspace_bytes(&G, 0), 0);
    EXPECT_EQ(codec_pee_volume_workspace_bytes(&G, 65), 0);
    EXPECT_EQ(codec_pee_volume_workspace_bytes(&G, -1), 0);
    EXPECT_EQ(codec_pee_volume_workspace_bytes(&G, INT32_MIN), 0);

    // ---- bad parameter sets: every entry
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_EQ(codec_pee_volume_workspace_bytes(B, 16), 0);
        EXPECT_NEG(codec_pee_volume_plan(B, i32, 16, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
        EXPECT_NEG(codec_pee_volume_scatter(B, u64p, 63, i32, i32, u64p, nullptr));
        EXPECT_NEG(codec_pee_volume_gather(B, meta, u64p, u64p, 1, i32, p, big, nullptr));
        EXPECT_NEG(codec_pee_volume_embed(B, p, p, u64p, 63, CODEC_VOL_EVEN, 16, i32, i32, i32, info, meta, u64p, p, big,
                                          p, big, nullptr));
        EXPECT_NEG(codec_pee_volume_extract(B, p, meta, u64p, p, u64p, 1, i32, p, big, p, big, nullptr));
    }
    EXPECT_NEG(codec_pee_volume_plan(nullptr, i32, 16, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(nullptr, u64p, 63, i32, i32, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(nullptr, meta, u64p, u64p, 1, i32, p, big, nullptr));
    EXPECT_NEG(codec_pee_volume_embed(nullptr, p, p, u64p, 63, CODEC_VOL_EVEN, 16, i32, i32, i32, info, meta, u64p, p, big,
                                      p, big, nullptr));
    EXPECT_NEG(codec_pee_volume_extract(nullptr, p, meta, u64p, p, u64p, 1, i32, p, big, p, big, nullptr));

    // ---- codec_pee_volume_plan
    EXPECT_NEG(codec_pee_volume_plan(&G, nullptr, 16, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, CODEC_VOL_EVEN, nullptr, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, CODEC_VOL_EVEN, i32, nullptr, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, CODEC_VOL_EVEN, i32, i32, nullptr, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, CODEC_VOL_EVEN, i32, i32, i32, nullptr, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 0, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 65, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, INT32_MIN, 63, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, -1, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, (int64_t)1 << 31, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, INT64_MAX, CODEC_VOL_FILL, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, INT64_MIN, CODEC_VOL_FILL, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, 2, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 63, -1, i32, i32, i32, info, nullptr));
    EXPECT_NEG(codec_pee_volume_plan(&G, i32, 16, 257, CODEC_VOL_EVEN, i32, i32, i32, info, nullptr));   // 4 words hold 256

    // ---- codec_pee_volume_scatter
    EXPECT_NEG(codec_pee_volume_scatter(&G, nullptr, 63, i32, i32, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, 63, nullptr, i32, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, 63, i32, nullptr, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, 63, i32, i32, nullptr, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, -1, i32, i32, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, (int64_t)1 << 31, i32, i32, u64p, nullptr));
    EXPECT_NEG(codec_pee_volume_scatter(&G, u64p, INT64_MAX, i32, i32, u64p, nullptr));

    // ---- codec_pee_volume_gather
    EXPECT_NEG(codec_pee_volume_gather(&G, nullptr, u64p, u64p, 1, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, nullptr, u64p, 1, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, nullptr, 1, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, 1, nullptr, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, 1, i32, nullptr, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, -1, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, ((int64_t)1 << 25) + 1, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, INT64_MAX, i32, p, vws1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, 1, i32, p, vws1 - 1, nullptr));
    EXPECT_NEG(codec_pee_volume_gather(&G, meta, u64p, u64p, 1, i32, p, 0, nullptr));

    // ---- codec_pee_volume_embed
#define EMBED(cover, stego, bits, N, pol, tmax, n, t, off, inf, m, lm, pw, pwb, vw, vwb) \
    codec_pee_volume_embed(&G, cover, stego, bits, N, pol, tmax, n, t, off, inf, m, lm, pw, pwb, vw, vwb, nullptr)
    EXPECT_NEG(EMBED(nullptr, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, nullptr, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, nullptr, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, nullptr, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, nullptr, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, nullptr, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, nullptr, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, nullptr, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, nullptr, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, nullptr, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, nullptr, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws - 1, p, vws));     // short workspaces
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, 0, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws - 1));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws1));        // sized for tmax = 1
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, 0));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 0, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 0, 65, i32, i32, i32, info, meta, u64p, p, pws, p, big));
    EXPECT_NEG(EMBED(p, p, u64p, 63, 2, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 63, -7, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, -1, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, (int64_t)1 << 31, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, INT64_MAX, 1, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));
    EXPECT_NEG(EMBED(p, p, u64p, 257, 0, 16, i32, i32, i32, info, meta, u64p, p, pws, p, vws));        // row pitch too small
#undef EMBED

    // ---- codec_pee_volume_extract
#define EXTRACT(stego, m, lm, cover, bits, sw, tot, pw, pwb, vw, vwb) \
    codec_pee_volume_extract(&G, stego, m, lm, cover, bits, sw, tot, pw, pwb, vw, vwb, nullptr)
    EXPECT_NEG(EXTRACT(nullptr, meta, u64p, p, u64p, 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, nullptr, u64p, p, u64p, 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, nullptr, p, u64p, 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, nullptr, u64p, 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, nullptr, 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, nullptr, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, i32, nullptr, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, i32, p, pws, nullptr, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, -1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, ((int64_t)1 << 25) + 1, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, INT64_MIN, i32, p, pws, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, i32, p, pws - 1, p, vws1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, i32, p, pws, p, vws1 - 1));
    EXPECT_NEG(EXTRACT(p, meta, u64p, p, u64p, 1, i32, p, 0, p, 0));
#undef EXTRACT

    expect_no_device_ops();
    return abi_report("abi_args_vol");
}

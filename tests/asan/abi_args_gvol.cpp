// Host sanitizer check of the argument validation of include/codec_tcc_gvol.h's entries, as
// abi_args_vol.cpp is for codec_tcc_vol.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status (0 for the size query) with an error text and no device operation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_gvol.h"

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
    P = good(); P.B = 1; P.H = 16386; P.W = 16384; P.lm_words = (8193 * 8192 + 63) / 64; out[k++] = P;   // 2^26 + 8192 candidates
    return k;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    uint64_t* u64p = reinterpret_cast<uint64_t*>(buf);
    codec_pee_meta* meta = reinterpret_cast<codec_pee_meta*>(buf);
    codec_pee_gvol_info* info = reinterpret_cast<codec_pee_gvol_info*>(buf);
    const size_t big = (size_t)1 << 40;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }
    if (sizeof(codec_pee_gvol_info) != 40 || sizeof(codec_pee_gvol_info) % 8) { fprintf(stderr, "FAIL info size\n"); ++g_fail; }

    codec_pee_params G = good();
    const size_t pws = codec_pee_workspace_bytes(&G);
    const size_t tws = codec_pee_gate_workspace_bytes(&G, 16);
    const size_t gws = codec_pee_gvol_workspace_bytes(&G, 16);
    const size_t gws1 = codec_pee_gvol_workspace_bytes(&G, 1);
    if (!pws || tws <= pws) { fprintf(stderr, "FAIL pee / gate workspace_bytes of good arguments\n"); ++g_fail; }
    if (gws < 5 * 17 * 16 * 4 + 5 * 4 * 8 + 6 * 4 || gws1 < 5 * 2 * 16 * 4 + 5 * 4 * 8 + 6 * 4 || gws1 > gws ||
        gws1 < codec_pee_volume_workspace_bytes(&G, 1)) {
        fprintf(stderr, "FAIL gated volume workspace_bytes of good arguments: %zu / %zu\n", gws, gws1);
        ++g_fail;
    }

    // ---- the size query
    EXPECT_EQ(codec_pee_gvol_workspace_bytes(nullptr, 16), 0);
    EXPECT_EQ(codec_pee_gvol_workspace_bytes(&G, 0), 0);
    EXPECT_EQ(codec_pee_gvol_workspace_bytes(&G, 17), 0);
    EXPECT_EQ(codec_pee_gvol_workspace_bytes(&G, -1), 0);
    EXPECT_EQ(codec_pee_gvol_workspace_bytes(&G, INT32_MIN), 0);

#define PLAN(Pp, n, hs, tmax, N, pol, g, no, to, go, oo, inf) \
    codec_pee_gvol_plan(Pp, n, hs, tmax, N, pol, g, no, to, go, oo, inf, nullptr)
#define EMBED(Pp, cover, stego, bits, N, pol, tmax, g, n, t, go, off, inf, m, lm, pw, pwb, tw, twb, gw, gwb) \
    codec_pee_gvol_embed(Pp, cover, stego, bits, N, pol, tmax, g, n, t, go, off, inf, m, lm, pw, pwb, tw, twb, gw, gwb, nullptr)
#define EXTRACT(Pp, stego, m, lm, cover, bits, sw, tot, pw, pwb, gw, gwb) \
    codec_pee_gvol_extract(Pp, stego, m, lm, cover, bits, sw, tot, pw, pwb, gw, gwb, nullptr)

    // ---- bad parameter sets: every entry
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_EQ(codec_pee_gvol_workspace_bytes(B, 16), 0);
        EXPECT_NEG(PLAN(B, u32, u32, 16, 63, CODEC_VOL_EVEN, -1, i32, i32, i32, i32, info));
        EXPECT_NEG(EMBED(B, p, p, u64p, 63, CODEC_VOL_EVEN, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, big, p, big, p, big));
        EXPECT_NEG(EXTRACT(B, p, meta, u64p, p, u64p, 1, i32, p, big, p, big));
    }
    EXPECT_NEG(PLAN(nullptr, u32, u32, 16, 63, CODEC_VOL_EVEN, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(EMBED(nullptr, p, p, u64p, 63, CODEC_VOL_EVEN, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, big, p, big, p, big));
    EXPECT_NEG(EXTRACT(nullptr, p, meta, u64p, p, u64p, 1, i32, p, big, p, big));

    // ---- codec_pee_gvol_plan
    EXPECT_NEG(PLAN(&G, nullptr, u32, 16, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, nullptr, 16, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -1, nullptr, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -1, i32, nullptr, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -1, i32, i32, nullptr, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -1, i32, i32, i32, nullptr, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -1, i32, i32, i32, i32, nullptr));
    EXPECT_NEG(PLAN(&G, u32, u32, 0, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 17, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 64, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, INT32_MIN, 63, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, -1, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, (int64_t)1 << 31, 0, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, INT64_MAX, 1, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, INT64_MIN, 1, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 2, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, -1, -1, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, -2, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, 65536, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 63, 0, INT32_MIN, i32, i32, i32, i32, info));
    EXPECT_NEG(PLAN(&G, u32, u32, 16, 257, 0, -1, i32, i32, i32, i32, info));   // 4 words hold 256

    // ---- codec_pee_gvol_embed
#define E(cover, stego, bits, N, pol, tmax, g, n, t, go, off, inf, m, lm, pw, pwb, tw, twb, gw, gwb) \
    EXPECT_NEG(EMBED(&G, cover, stego, bits, N, pol, tmax, g, n, t, go, off, inf, m, lm, pw, pwb, tw, twb, gw, gwb))
    E(nullptr, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, nullptr, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, nullptr, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, nullptr, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, nullptr, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, nullptr, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, nullptr, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, nullptr, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, nullptr, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, nullptr, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, nullptr, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, nullptr, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, nullptr, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws - 1, p, tws, p, gws);   // short workspaces
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, 0, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws - 1, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, pws, p, gws);       // no room for the bins
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, 0, p, gws);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws - 1);
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws1);      // sized for tmax = 1
    E(p, p, u64p, 63, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, 0);
    E(p, p, u64p, 63, 0, 0, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 17, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, big, p, big);
    E(p, p, u64p, 63, 2, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, -7, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, -2, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 63, 0, 16, 65536, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, -1, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, (int64_t)1 << 31, 0, 16, -1, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, INT64_MAX, 1, 16, 6, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);
    E(p, p, u64p, 257, 0, 16, 6, i32, i32, i32, i32, info, meta, u64p, p, pws, p, tws, p, gws);       // row pitch too small
#undef E

    // ---- codec_pee_gvol_extract
#define X(stego, m, lm, cover, bits, sw, tot, pw, pwb, gw, gwb) \
    EXPECT_NEG(EXTRACT(&G, stego, m, lm, cover, bits, sw, tot, pw, pwb, gw, gwb))
    X(nullptr, meta, u64p, p, u64p, 1, i32, p, pws, p, gws1);
    X(p, nullptr, u64p, p, u64p, 1, i32, p, pws, p, gws1);
    X(p, meta, nullptr, p, u64p, 1, i32, p, pws, p, gws1);
    X(p, meta, u64p, nullptr, u64p, 1, i32, p, pws, p, gws1);
    X(p, meta, u64p, p, nullptr, 1, i32, p, pws, p, gws1);
    X(p, meta, u64p, p, u64p, 1, nullptr, p, pws, p, gws1);
    X(p, meta, u64p, p, u64p, 1, i32, nullptr, pws, p, gws1);
    X(p, meta, u64p, p, u64p, 1, i32, p, pws, nullptr, gws1);
    X(p, meta, u64p, p, u64p, -1, i32, p, pws, p, gws1);
    X(p, meta, u64p, p, u64p, ((int64_t)1 << 25) + 1, i32, p, pws, p, gws1);
    X(p, meta, u64p, p, u64p, INT64_MIN, i32, p, pws, p, gws1);
    X(p, meta, u64p, p, u64p, 1, i32, p, pws - 1, p, gws1);
    X(p, meta, u64p, p, u64p, 1, i32, p, pws, p, gws1 - 1);
    X(p, meta, u64p, p, u64p, 1, i32, p, 0, p, 0);
#undef X

    expect_no_device_ops();
    return abi_report("abi_args_gvol");
}

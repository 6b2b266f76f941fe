// Host sanitizer check of the argument validation of include/codec_tcc_gate.h's entries, as
// abi_args_vol.cpp is for codec_tcc_vol.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status (0 for the size query) with an error text and no device operation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_gate.h"

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
    return k;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    uint64_t* u64p = reinterpret_cast<uint64_t*>(buf);
    codec_pee_meta* meta = reinterpret_cast<codec_pee_meta*>(buf);
    const size_t big = (size_t)1 << 40;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }

    codec_pee_params G = good();
    const size_t pws = codec_pee_workspace_bytes(&G);
    const size_t gws = codec_pee_gate_workspace_bytes(&G, 16);
    if (!pws || gws < pws + 5 * (17 * 16 + 1) * 4) {
        fprintf(stderr, "FAIL workspace sizes of good arguments: %zu / %zu\n", pws, gws);
        ++g_fail;
    }
    EXPECT_EQ(codec_pee_gate_workspace_bytes(&G, 1), gws);   // the tail does not depend on tmax

    // ---- the size query
    EXPECT_EQ(codec_pee_gate_workspace_bytes(nullptr, 16), 0);
    EXPECT_EQ(codec_pee_gate_workspace_bytes(&G, 0), 0);
    EXPECT_EQ(codec_pee_gate_workspace_bytes(&G, 17), 0);
    EXPECT_EQ(codec_pee_gate_workspace_bytes(&G, -1), 0);
    EXPECT_EQ(codec_pee_gate_workspace_bytes(&G, INT32_MIN), 0);

#define CAP(P, cover, tmax, tf, gf, len, n, hs, t, g, k, ws, wsb) \
    codec_pee_gate_capacity(P, cover, tmax, tf, gf, len, n, hs, t, g, k, ws, wsb, nullptr)
#define EMB(P, cover, stego, pay, len, t, g, m, lm, ws, wsb) \
    codec_pee_gate_embed(P, cover, stego, pay, len, t, g, m, lm, ws, wsb, nullptr)
#define AUTO(P, cover, stego, pay, len, tmax, tf, gf, t, g, m, lm, ws, wsb) \
    codec_pee_gate_embed_auto(P, cover, stego, pay, len, tmax, tf, gf, t, g, m, lm, ws, wsb, nullptr)
#define EXT(P, stego, m, lm, cover, pay, ws, wsb) codec_pee_gate_extract(P, stego, m, lm, cover, pay, ws, wsb, nullptr)

    // ---- bad parameter sets: every entry
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_EQ(codec_pee_gate_workspace_bytes(B, 16), 0);
        EXPECT_NEG(CAP(B, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, big));
        EXPECT_NEG(EMB(B, p, p, u64p, i32, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(AUTO(B, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EXT(B, p, meta, u64p, p, u64p, p, big));
    }
    EXPECT_NEG(CAP(nullptr, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, big));
    EXPECT_NEG(EMB(nullptr, p, p, u64p, i32, i32, i32, meta, u64p, p, big));
    EXPECT_NEG(AUTO(nullptr, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, big));
    EXPECT_NEG(EXT(nullptr, p, meta, u64p, p, u64p, p, big));
    // more than 2^26 candidates per slice: the table and the selection refuse, the size query too
    {
        codec_pee_params P = good();
        P.B = 1; P.H = 16386; P.W = 16386; P.lm_words = (8193 * 8193 + 63) / 64;
        EXPECT_EQ(codec_pee_gate_workspace_bytes(&P, 16), 0);
        EXPECT_NEG(CAP(&P, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, big));
        EXPECT_NEG(AUTO(&P, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, big));
    }

    // ---- codec_pee_gate_capacity
    EXPECT_NEG(CAP(&G, nullptr, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, nullptr, gws));
    EXPECT_NEG(CAP(&G, p, 0, 0, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 17, 0, -1, i32, u32, u32, i32, i32, i32, p, big));
    EXPECT_NEG(CAP(&G, p, -1, 0, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, INT32_MIN, 0, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, -1, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 17, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 4, 5, -1, i32, u32, u32, i32, i32, i32, p, gws));        // t_fixed above tmax
    EXPECT_NEG(CAP(&G, p, 16, INT32_MAX, -1, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, -2, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, 65536, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, INT32_MIN, i32, u32, u32, i32, i32, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, nullptr, u32, u32, i32, nullptr, nullptr, p, gws));   // outputs without lengths
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, nullptr, u32, u32, nullptr, i32, nullptr, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, nullptr, u32, u32, nullptr, nullptr, i32, p, gws));
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, gws - 1));      // short workspaces
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, pws));          // a codec_pee one: no tail
    EXPECT_NEG(CAP(&G, p, 16, 0, -1, i32, u32, u32, i32, i32, i32, p, 0));

    // ---- codec_pee_gate_embed
    EXPECT_NEG(EMB(&G, nullptr, p, u64p, i32, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, nullptr, u64p, i32, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, nullptr, i32, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, nullptr, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, nullptr, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, nullptr, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, i32, nullptr, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, i32, meta, nullptr, p, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, i32, meta, u64p, nullptr, pws));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, i32, meta, u64p, p, pws - 1));
    EXPECT_NEG(EMB(&G, p, p, u64p, i32, i32, i32, meta, u64p, p, 0));

    // ---- codec_pee_gate_embed_auto
    EXPECT_NEG(AUTO(&G, nullptr, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, nullptr, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, nullptr, i32, 16, 0, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, nullptr, 16, 0, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, nullptr, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, nullptr, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, nullptr, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, nullptr, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, nullptr, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 0, 0, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 17, 0, -1, i32, i32, meta, u64p, p, big));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 17, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, -1, -1, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, 65536, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -2, i32, i32, meta, u64p, p, gws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, gws - 1));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(AUTO(&G, p, p, u64p, i32, 16, 0, -1, i32, i32, meta, u64p, p, 0));

    // ---- codec_pee_gate_extract
    EXPECT_NEG(EXT(&G, nullptr, meta, u64p, p, u64p, p, pws));
    EXPECT_NEG(EXT(&G, p, nullptr, u64p, p, u64p, p, pws));
    EXPECT_NEG(EXT(&G, p, meta, nullptr, p, u64p, p, pws));
    EXPECT_NEG(EXT(&G, p, meta, u64p, nullptr, u64p, p, pws));
    EXPECT_NEG(EXT(&G, p, meta, u64p, p, nullptr, p, pws));
    EXPECT_NEG(EXT(&G, p, meta, u64p, p, u64p, nullptr, pws));
    EXPECT_NEG(EXT(&G, p, meta, u64p, p, u64p, p, pws - 1));
    EXPECT_NEG(EXT(&G, p, meta, u64p, p, u64p, p, 0));

    expect_no_device_ops();
    return abi_report("abi_args_gate");
}

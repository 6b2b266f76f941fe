// Host sanitizer check of the argument validation of include/codec_tcc_blind_gate.h's entries, as
// abi_args_blind_auto.cpp is for codec_tcc_blind_auto.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi_blind_gate.py builds and runs it).  Every bad call must return its negative
// status (0 for the size function) with an error text and no device operation; every call with
// good arguments must get past the checks, i.e. reach its first device operation (which the
// stubs refuse and count).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_blind_gate.h"

#include "abi_expect.h"

#define ME 8   // max_entries of the good calls: rows of (192 + 32 * 8 + 64 * 4 + 63) / 64 = 11 words
#define TM 8   // tmax of the good calls

static codec_pee_params good() {
    codec_pee_params P;
    memset(&P, 0, sizeof(P));
    P.B = 5; P.H = 64; P.W = 96; P.bytes = 2; P.T = 2; P.maxval = 4095;
    P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(256, ME); P.lm_words = 24;   // (64 / 2) * (96 / 2) = 1536 candidates
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
    P = good(); P.T = 0; out[k++] = P;                                             // only range-checked, but checked
    P = good(); P.T = 65; out[k++] = P;
    P = good(); P.maxval = 0; out[k++] = P;
    P = good(); P.maxval = 65536; out[k++] = P;
    P = good(); P.bytes = 1; P.maxval = 256; out[k++] = P;
    P = good(); P.payload_words = 0; out[k++] = P;
    P = good(); P.payload_words = -1; out[k++] = P;
    P = good(); P.lm_words = 0; out[k++] = P;
    P = good(); P.lm_words = 23; out[k++] = P;                                     // 1472 < 1536 candidates
    P = good(); P.H = 8; P.W = 16; P.lm_words = 1; out[k++] = P;                   // 128 pixels: no room for 192 header bits
    return k;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    void* q = buf + 32768;
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    uint64_t* u64p = reinterpret_cast<uint64_t*>(buf);
    codec_pee_meta* meta = reinterpret_cast<codec_pee_meta*>(buf);
    const size_t big = (size_t)1 << 40;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }

    codec_pee_params G = good();
    const size_t pws = codec_pee_workspace_bytes(&G);
    const size_t fws = codec_pee_blind_workspace_bytes(&G, ME);
    const size_t aws = codec_pee_blind_gate_workspace_bytes(&G, TM, ME);
    const size_t aws1 = codec_pee_blind_gate_workspace_bytes(&G, 1, ME);
    const size_t aws16 = codec_pee_blind_gate_workspace_bytes(&G, 16, ME);
    // every T adds a table of B * 16 * hc words, rounded up to 256 bytes once; one flag word per slice behind it
    if (!pws || aws1 <= fws || aws <= aws1 || aws16 <= aws || aws - aws1 < (size_t)(TM - 1) * 5 * 16 * 32 * 4 - 255 ||
        aws - aws1 > (size_t)(TM - 1) * 5 * 16 * 32 * 4 + 255) {
        fprintf(stderr, "FAIL workspace sizes of good arguments: %zu / %zu / %zu / %zu / %zu\n", pws, fws, aws1, aws, aws16);
        ++g_fail;
    }

#define WSB(P, tm, me) codec_pee_blind_gate_workspace_bytes(P, tm, me)
#define PLANF(P, cover, len, tm, tf, jf, me, info, tout, gout, curve, ws, wsb) \
    codec_pee_blind_plan_gate(P, cover, len, tm, tf, jf, me, info, tout, gout, curve, ws, wsb, nullptr)
#define EMBF(P, cover, stego, pay, uw, len, crc, tm, tf, jf, me, info, tout, gout, m, lm, ws, wsb) \
    codec_pee_blind_embed_gate(P, cover, stego, pay, uw, len, crc, tm, tf, jf, me, info, tout, gout, m, lm, ws, wsb, nullptr)
// with both free, and g_out beside t_out
#define PLAN(P, cover, len, tm, me, info, tout, curve, ws, wsb) PLANF(P, cover, len, tm, 0, -1, me, info, tout, tout, curve, ws, wsb)
#define EMB(P, cover, stego, pay, uw, len, crc, tm, me, info, tout, m, lm, ws, wsb) \
    EMBF(P, cover, stego, pay, uw, len, crc, tm, 0, -1, me, info, tout, tout, m, lm, ws, wsb)

    // ---- bad parameter sets: every entry
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_EQ(WSB(B, TM, ME), 0);
        EXPECT_NEG(PLAN(B, p, i32, TM, ME, i32, i32, i32, p, big));
        EXPECT_NEG(PLAN(B, p, nullptr, TM, ME, i32, i32, nullptr, p, big));
        EXPECT_NEG(EMB(B, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EMB(B, p, q, u64p, 4, i32, nullptr, TM, ME, i32, i32, meta, u64p, p, big));
    }
    EXPECT_EQ(WSB(nullptr, TM, ME), 0);
    EXPECT_NEG(PLAN(nullptr, p, i32, TM, ME, i32, i32, i32, p, big));
    EXPECT_NEG(EMB(nullptr, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, big));
    // H or W above 65535: the reserved rectangle travels in the ROI record words
    for (int k = 0; k < 2; ++k) {
        codec_pee_params P = good();
        P.B = 1;
        if (k == 0) { P.H = 65536; P.W = 8; } else { P.H = 8; P.W = 65536; }
        P.lm_words = (4 * 32768 + 63) / 64;
        if (!codec_pee_workspace_bytes(&P)) { fprintf(stderr, "FAIL: the tall / wide shape is not a codec_pee one\n"); ++g_fail; }
        EXPECT_EQ(WSB(&P, TM, ME), 0);
        EXPECT_NEG(PLAN(&P, p, i32, TM, ME, i32, i32, i32, p, big));
        EXPECT_NEG(EMB(&P, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, big));
    }
    // tmax outside 1..16
    for (int32_t tm : {0, -1, 17, 64, INT32_MIN, INT32_MAX}) {
        EXPECT_EQ(WSB(&G, tm, ME), 0);
        EXPECT_NEG(PLAN(&G, p, i32, tm, ME, i32, i32, i32, p, big));
        EXPECT_NEG(PLAN(&G, p, nullptr, tm, ME, i32, i32, nullptr, p, big));
        EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, tm, ME, i32, i32, meta, u64p, p, big));
    }
    // t_fixed outside 0..tmax, j_fixed outside -1..15
    for (int32_t tf : {-1, TM + 1, 17, INT32_MIN, INT32_MAX}) {
        EXPECT_NEG(PLANF(&G, p, i32, TM, tf, -1, ME, i32, i32, i32, i32, p, big));
        EXPECT_NEG(EMBF(&G, p, q, u64p, 4, i32, u32, TM, tf, -1, ME, i32, i32, i32, meta, u64p, p, big));
    }
    for (int32_t jf : {-2, 16, 65535, INT32_MIN, INT32_MAX}) {
        EXPECT_NEG(PLANF(&G, p, i32, TM, 0, jf, ME, i32, i32, i32, i32, p, big));
        EXPECT_NEG(EMBF(&G, p, q, u64p, 4, i32, u32, TM, 0, jf, ME, i32, i32, i32, meta, u64p, p, big));
    }
    // g_out NULL
    EXPECT_NEG(PLANF(&G, p, i32, TM, 0, -1, ME, i32, i32, nullptr, i32, p, big));
    EXPECT_NEG(EMBF(&G, p, q, u64p, 4, i32, u32, TM, 0, -1, ME, i32, i32, nullptr, meta, u64p, p, big));
    // max_entries out of range, and rows narrower than its side bits
    for (int32_t me : {-1, INT32_MIN, CODEC_PEE_BLIND_MAX_ENTRIES + 1, INT32_MAX}) {
        EXPECT_EQ(WSB(&G, TM, me), 0);
        EXPECT_NEG(PLAN(&G, p, i32, TM, me, i32, i32, i32, p, big));
        EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, me, i32, i32, meta, u64p, p, big));
    }
    {
        codec_pee_params P = good();
        P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(0, ME) - 1;
        EXPECT_EQ(WSB(&P, TM, ME), 0);
        EXPECT_NEG(PLAN(&P, p, i32, TM, ME, i32, i32, i32, p, big));
        EXPECT_NEG(EMB(&P, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, big));
    }

    // ---- codec_pee_blind_plan_gate
    EXPECT_NEG(PLAN(&G, nullptr, i32, TM, ME, i32, i32, i32, p, aws));
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, nullptr, i32, i32, p, aws));
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, i32, nullptr, i32, p, aws));
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, i32, i32, i32, nullptr, aws));
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, i32, i32, i32, p, aws - 1));
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, i32, i32, i32, p, fws));       // the fixed workspace: no table of pairs
    EXPECT_NEG(PLAN(&G, p, i32, 16, ME, i32, i32, i32, p, aws));       // sized for TM, asked for 16
    EXPECT_NEG(PLAN(&G, p, i32, TM, ME, i32, i32, i32, p, pws));
    EXPECT_NEG(PLAN(&G, p, nullptr, TM, ME, i32, i32, nullptr, p, 0));

    // ---- codec_pee_blind_embed_gate
    EXPECT_NEG(EMB(&G, nullptr, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, nullptr, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, nullptr, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, nullptr, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, nullptr, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, nullptr, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, nullptr, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, nullptr, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, nullptr, aws));
    EXPECT_NEG(EMB(&G, p, p, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));            // in place
    EXPECT_NEG(EMB(&G, p, q, u64p, 0, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, -1, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, INT32_MAX, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, p, aws - 1));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, u32, 16, ME, i32, i32, meta, u64p, p, aws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, nullptr, TM, ME, i32, i32, meta, u64p, p, fws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, nullptr, TM, ME, i32, i32, meta, u64p, p, pws));
    EXPECT_NEG(EMB(&G, p, q, u64p, 4, i32, nullptr, TM, ME, i32, i32, meta, u64p, p, 0));

    expect_no_device_ops();

    // ---- good arguments: each entry gets past its checks and reaches a device operation, which
    // the stubs refuse and count.  The buffer stands in for device memory:
    // nothing dereferences it on the host.
    {
        static unsigned char ws[1 << 22];
        if (aws16 > sizeof(ws)) { fprintf(stderr, "FAIL: workspace of the good shape is %zu bytes\n", aws16); return 2; }
        g_ops = hip_stub_device_ops();
        EXPECT_REACHED(PLAN(&G, p, i32, TM, ME, i32, i32, i32, ws, aws));
        EXPECT_REACHED(PLAN(&G, p, nullptr, 1, 0, i32, i32, nullptr, ws, aws));
        EXPECT_REACHED(PLAN(&G, buf + 2, nullptr, 16, ME, i32, i32, i32, ws, aws16));                  // an offset view
        EXPECT_REACHED(EMB(&G, p, q, u64p, 4, i32, u32, TM, ME, i32, i32, meta, u64p, ws, aws));
        EXPECT_REACHED(EMB(&G, buf + 2, q, u64p, 1, i32, nullptr, 1, 0, i32, i32, meta, u64p, ws, aws));
        EXPECT_REACHED(EMB(&G, p, q, u64p, 4, i32, u32, 16, ME, i32, i32, meta, u64p, ws, aws16));
        EXPECT_REACHED(PLANF(&G, p, i32, TM, TM, 15, ME, i32, i32, i32, i32, ws, aws));               // both fixed
        EXPECT_REACHED(PLANF(&G, p, i32, TM, 1, -1, ME, i32, i32, i32, nullptr, ws, aws));
        EXPECT_REACHED(EMBF(&G, p, q, u64p, 4, i32, u32, TM, 0, 0, ME, i32, i32, i32, meta, u64p, ws, aws));
        EXPECT_REACHED(EMBF(&G, p, q, u64p, 4, i32, nullptr, TM, 3, 7, ME, i32, i32, i32, meta, u64p, ws, aws));
    }
    return abi_report("abi_args_blind_gate");
}

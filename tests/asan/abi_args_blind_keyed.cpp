// Host sanitizer check of the argument validation of include/codec_tcc_blind_keyed.h's entries, as
// abi_args_blind_auto.cpp is for codec_tcc_blind_auto.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi_blind_keyed.py builds and runs it).  Every bad call must return its negative
// status with an error text and no device operation; every call with good arguments must get past
// the checks, i.e. reach its first device operation (which the stubs refuse and count).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_blind_keyed.h"

#include "abi_expect.h"

#define ME 8   // max_entries of the good calls
#define TM 8   // tmax of the good calls that choose T
#define CW 4   // ciphertext words of the good calls

static codec_pee_params good() {
    codec_pee_params P;
    memset(&P, 0, sizeof(P));
    P.B = 5; P.H = 64; P.W = 96; P.bytes = 2; P.T = 2; P.maxval = 4095;
    P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(64 * CW + CODEC_PEE_BLIND_FRAME_BITS, ME); P.lm_words = 24;
    return P;
}

// the parameter sets the embed must refuse
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
    P = good(); P.T = 65; out[k++] = P;
    P = good(); P.maxval = 0; out[k++] = P;
    P = good(); P.maxval = 65536; out[k++] = P;
    P = good(); P.bytes = 1; P.maxval = 256; out[k++] = P;
    P = good(); P.payload_words = 0; out[k++] = P;
    P = good(); P.payload_words = -1; out[k++] = P;
    P = good(); P.lm_words = 0; out[k++] = P;
    P = good(); P.lm_words = 23; out[k++] = P;                                     // 1472 < 1536 candidates
    P = good(); P.H = 8; P.W = 16; P.lm_words = 1; out[k++] = P;                   // 128 pixels: no room for 192 header bits
    P = good(); P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(0, ME) - 1; out[k++] = P;   // below the side bits
    P = good(); P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(CODEC_PEE_BLIND_FRAME_BITS, ME) - 1; out[k++] = P;   // no room for the frame
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
    const codec_aead_ctx* ctx = reinterpret_cast<const codec_aead_ctx*>(buf);
    const size_t big = (size_t)1 << 40;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }

    codec_pee_params G = good();
    const size_t pws = codec_pee_workspace_bytes(&G);
    const size_t fws = codec_pee_blind_workspace_bytes(&G, ME);
    const size_t aws = codec_pee_blind_auto_workspace_bytes(&G, TM, ME);
    const size_t aws16 = codec_pee_blind_auto_workspace_bytes(&G, 16, ME);
    const size_t tws = codec_aead_workspace_bytes(5, 64 * 96 * 2, CW);
    if (!pws || !fws || aws <= fws || aws16 <= aws || !tws) {
        fprintf(stderr, "FAIL workspace sizes of good arguments: %zu / %zu / %zu / %zu / %zu\n", pws, fws, aws, aws16, tws);
        ++g_fail;
    }

#define EMB(P, cover, stego, fr, ct, cw, len, tm, me, info, ts, m, lm, ws, wsb) \
    codec_pee_blind_embed_keyed(P, cover, stego, fr, ct, cw, len, tm, me, info, ts, m, lm, ws, wsb, nullptr)
#define ROWS(c, B, n, in, rw, len, out) codec_chacha20_rows_n(c, B, n, in, rw, len, out, nullptr)
#define TAGS(c, B, n, aad, ab, ct, rw, len, tags, ws, wsb) codec_poly1305_tags_n(c, B, n, aad, ab, ct, rw, len, tags, ws, wsb, nullptr)
#define REL(c, B, n, tg, tw, ct, rw, len, out, ok) codec_aead_release_n(c, B, n, tg, tw, ct, rw, len, out, ok, nullptr)
#define FRM(c, B, i0, tags, out) codec_pee_blind_frames(c, B, i0, tags, out, nullptr)
#define UNF(B, rows, uw, hdr, n, t, ct, cw, len) codec_pee_blind_unframe(B, rows, uw, hdr, n, t, ct, cw, len, nullptr)

    // ---- codec_pee_blind_embed_keyed: bad parameter sets, fixed T and chosen T
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_NEG(EMB(B, p, q, u32, u64p, CW, i32, 0, ME, i32, nullptr, meta, u64p, p, big));
        EXPECT_NEG(EMB(B, p, q, u32, u64p, CW, i32, 0, ME, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EMB(B, p, q, u32, u64p, CW, i32, TM, ME, i32, i32, meta, u64p, p, big));
    }
    EXPECT_NEG(EMB(nullptr, p, q, u32, u64p, CW, i32, 0, ME, i32, i32, meta, u64p, p, big));
    EXPECT_NEG(EMB(nullptr, p, q, u32, u64p, CW, i32, TM, ME, i32, i32, meta, u64p, p, big));
    for (int k = 0; k < 2; ++k) {   // H or W above 65535: the reserved rectangle travels in the ROI record words
        codec_pee_params P = good();
        P.B = 1;
        if (k == 0) { P.H = 65536; P.W = 8; } else { P.H = 8; P.W = 65536; }
        P.lm_words = (4 * 32768 + 63) / 64;
        if (!codec_pee_workspace_bytes(&P)) { fprintf(stderr, "FAIL: the tall / wide shape is not a codec_pee one\n"); ++g_fail; }
        EXPECT_NEG(EMB(&P, p, q, u32, u64p, CW, i32, 0, ME, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EMB(&P, p, q, u32, u64p, CW, i32, TM, ME, i32, i32, meta, u64p, p, big));
    }
    for (int32_t tm : {-1, 17, 64, INT32_MIN, INT32_MAX})   // tmax outside 0..16
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, big));
    for (int32_t me : {-1, INT32_MIN, CODEC_PEE_BLIND_MAX_ENTRIES + 1, INT32_MAX}) {
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, 0, me, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, TM, me, i32, i32, meta, u64p, p, big));
    }
    for (int32_t tm : {0, TM}) {   // NULL pointers, the call's own rules, the workspace
        const size_t ws = tm ? aws : fws;
        EXPECT_NEG(EMB(&G, nullptr, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, nullptr, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, nullptr, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, nullptr, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, nullptr, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, nullptr, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, nullptr, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, nullptr, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, nullptr, ws));
        EXPECT_NEG(EMB(&G, p, p, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws));            // in place
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, 0, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, -1, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, INT32_MAX, i32, tm, ME, i32, i32, meta, u64p, p, ws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, ws - 1));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, pws));
        EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, tm, ME, i32, i32, meta, u64p, p, 0));
    }
    EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, TM, ME, i32, nullptr, meta, u64p, p, aws));   // ts is needed when T is chosen
    EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, TM, ME, i32, i32, meta, u64p, p, fws));       // the fixed workspace: tables short
    EXPECT_NEG(EMB(&G, p, q, u32, u64p, CW, i32, 16, ME, i32, i32, meta, u64p, p, aws));       // sized for TM, asked for 16

    // ---- codec_chacha20_rows_n / codec_aead_release_n
    for (int32_t B : {0, -1, INT32_MIN}) {
        EXPECT_NEG(ROWS(ctx, B, u32, u64p, CW, i32, u64p));
        EXPECT_NEG(REL(ctx, B, u32, u32, u32, u64p, CW, i32, u64p, i32));
    }
    for (int32_t rw : {0, -1, CODEC_AEAD_MAX_ROW_WORDS + 1, INT32_MAX}) {
        EXPECT_NEG(ROWS(ctx, 5, u32, u64p, rw, i32, u64p));
        EXPECT_NEG(REL(ctx, 5, u32, u32, u32, u64p, rw, i32, u64p, i32));
    }
    EXPECT_NEG(ROWS(ctx, INT32_MAX, u32, u64p, CODEC_AEAD_MAX_ROW_WORDS, i32, u64p));   // past the grid limit
    EXPECT_NEG(ROWS(nullptr, 5, u32, u64p, CW, i32, u64p));
    EXPECT_NEG(ROWS(ctx, 5, nullptr, u64p, CW, i32, u64p));
    EXPECT_NEG(ROWS(ctx, 5, u32, nullptr, CW, i32, u64p));
    EXPECT_NEG(ROWS(ctx, 5, u32, u64p, CW, nullptr, u64p));
    EXPECT_NEG(ROWS(ctx, 5, u32, u64p, CW, i32, nullptr));
    EXPECT_NEG(REL(nullptr, 5, u32, u32, u32, u64p, CW, i32, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, nullptr, u32, u32, u64p, CW, i32, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, u32, nullptr, u32, u64p, CW, i32, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, u32, u32, nullptr, u64p, CW, i32, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, u32, u32, u32, nullptr, CW, i32, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, u32, u32, u32, u64p, CW, nullptr, u64p, i32));
    EXPECT_NEG(REL(ctx, 5, u32, u32, u32, u64p, CW, i32, nullptr, i32));
    EXPECT_NEG(REL(ctx, 5, u32, u32, u32, u64p, CW, i32, u64p, nullptr));

    // ---- codec_poly1305_tags_n
    const int64_t AB = 64 * 96 * 2;
    EXPECT_NEG(TAGS(ctx, 0, u32, p, AB, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, -1, u32, p, AB, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, -1, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, ((int64_t)1 << 32) + 1, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, nullptr, AB, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, 0, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, 0, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, nullptr, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CW, nullptr, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, -1, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CODEC_AEAD_MAX_ROW_WORDS + 1, i32, u32, q, big));
    EXPECT_NEG(TAGS(nullptr, 5, u32, p, AB, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, nullptr, p, AB, u64p, CW, i32, u32, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CW, i32, nullptr, q, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CW, i32, u32, nullptr, big));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CW, i32, u32, q, tws - 1));
    EXPECT_NEG(TAGS(ctx, 5, u32, p, AB, u64p, CW, i32, u32, q, 0));

    // ---- codec_pee_blind_frames
    for (int32_t B : {0, -1, INT32_MIN}) EXPECT_NEG(FRM(ctx, B, 0u, u32, u32));
    EXPECT_NEG(FRM(ctx, 5, 0x7FFFFFFCu, u32, u32));                      // the last index would be 2^31
    EXPECT_NEG(FRM(ctx, 2, CODEC_AEAD_STREAM_INDEX, u32, u32));
    EXPECT_NEG(FRM(ctx, 1, CODEC_AEAD_STREAM_INDEX + 1u, u32, u32));
    EXPECT_NEG(FRM(ctx, 1, 0xFFFFFFFFu, u32, u32));
    EXPECT_NEG(FRM(nullptr, 5, 0u, u32, u32));
    EXPECT_NEG(FRM(ctx, 5, 0u, nullptr, u32));
    EXPECT_NEG(FRM(ctx, 5, 0u, u32, nullptr));

    // ---- codec_pee_blind_unframe
    for (int32_t B : {0, -1, 65536, INT32_MIN, INT32_MAX}) EXPECT_NEG(UNF(B, u64p, 8, u32, u32, u32, u64p, CW, i32));
    for (int32_t w : {0, -1, (1 << 24) + 1, INT32_MIN, INT32_MAX}) {
        EXPECT_NEG(UNF(5, u64p, w, u32, u32, u32, u64p, CW, i32));
        EXPECT_NEG(UNF(5, u64p, 8, u32, u32, u32, u64p, w, i32));
    }
    EXPECT_NEG(UNF(5, nullptr, 8, u32, u32, u32, u64p, CW, i32));
    EXPECT_NEG(UNF(5, u64p, 8, nullptr, u32, u32, u64p, CW, i32));
    EXPECT_NEG(UNF(5, u64p, 8, u32, nullptr, u32, u64p, CW, i32));
    EXPECT_NEG(UNF(5, u64p, 8, u32, u32, nullptr, u64p, CW, i32));
    EXPECT_NEG(UNF(5, u64p, 8, u32, u32, u32, nullptr, CW, i32));
    EXPECT_NEG(UNF(5, u64p, 8, u32, u32, u32, u64p, CW, nullptr));

    expect_no_device_ops();

    // ---- good arguments: each entry gets past its checks and reaches a device operation, which
    // the stubs refuse and count.  The buffers stand in for device memory: nothing dereferences
    // them on the host.
    {
        static unsigned char ws[1 << 22];
        if (aws16 > sizeof(ws) || tws > sizeof(ws)) { fprintf(stderr, "FAIL: workspace of the good shape is %zu bytes\n", aws16); return 2; }
        g_ops = hip_stub_device_ops();
        EXPECT_REACHED(EMB(&G, p, q, u32, u64p, CW, i32, 0, ME, i32, nullptr, meta, u64p, ws, fws));   // fixed T: no ts
        EXPECT_REACHED(EMB(&G, p, q, u32, u64p, CW, i32, 0, ME, i32, i32, meta, u64p, ws, fws));
        EXPECT_REACHED(EMB(&G, buf + 2, q, u32, u64p, 1, i32, 1, 0, i32, i32, meta, u64p, ws, aws));   // an offset view
        EXPECT_REACHED(EMB(&G, p, q, u32, u64p, CW, i32, TM, ME, i32, i32, meta, u64p, ws, aws));
        EXPECT_REACHED(EMB(&G, p, q, u32, u64p, CW, i32, 16, ME, i32, i32, meta, u64p, ws, aws16));
        EXPECT_REACHED(ROWS(ctx, 5, u32, u64p, CW, i32, u64p));
        EXPECT_REACHED(ROWS(ctx, 1, u32, u64p, 1, i32, u64p + 64));
        EXPECT_REACHED(TAGS(ctx, 5, u32, p, AB, u64p, CW, i32, u32, ws, tws));
        EXPECT_REACHED(TAGS(ctx, 5, u32, nullptr, 0, u64p, CW, i32, u32, ws, tws));
        EXPECT_REACHED(TAGS(ctx, 5, u32, p, AB, nullptr, 0, nullptr, u32, ws, tws));
        EXPECT_REACHED(REL(ctx, 5, u32, u32, u32 + 64, u64p, CW, i32, u64p, i32));
        EXPECT_REACHED(FRM(ctx, 5, 0u, u32, u32 + 64));
        EXPECT_REACHED(FRM(ctx, 5, 0x7FFFFFFBu, u32, u32 + 64));          // the last index is 2^31 - 1
        EXPECT_REACHED(FRM(ctx, 1, CODEC_AEAD_STREAM_INDEX, u32, u32 + 64));
        EXPECT_REACHED(UNF(5, u64p, 8, u32, u32, u32, u64p, CW, i32));
        EXPECT_REACHED(UNF(65535, u64p, 1, u32, u32, u32, u64p, 1, i32));
    }
    return abi_report("abi_args_blind_keyed");
}

// Host sanitizer check of the argument validation of include/codec_tcc_blind_vol.h's entries, as
// abi_args_blind_keyed.cpp is for codec_tcc_blind_keyed.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi_blind_vol.py builds and runs it).  Every bad call must return its negative
// status (the workspace size: 0) with an error text and no device operation; every call with good
// arguments must get past the checks, i.e. reach its first device operation (which the stubs refuse
// and count).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_blind_vol.h"

#include "abi_expect.h"

#define ME 8    // max_entries of the good calls
#define TM 8    // tmax of the good calls
#define UW 12   // user-row words of the good decode-side calls
#define NB 3000 // stream bits of the good calls

static codec_pee_params good() {
    codec_pee_params P;
    memset(&P, 0, sizeof(P));
    P.B = 5; P.H = 64; P.W = 96; P.bytes = 2; P.T = 1; P.maxval = 4095;
    P.payload_words = (int32_t)CODEC_PEE_BLIND_ROW_WORDS(CODEC_PEE_BVOL_FRAME_BITS + 1536, ME); P.lm_words = 24;
    return P;
}

// the parameter sets every entry must refuse
static int bad_params(codec_pee_params* out) {
    int k = 0;
    codec_pee_params P;
    P = good(); P.B = 0; out[k++] = P;
    P = good(); P.B = -3; out[k++] = P;
    P = good(); P.B = INT32_MIN; out[k++] = P;
    P = good(); P.B = 65536; out[k++] = P;                                         // the frame holds 16 bits of B
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
    P = good(); P.payload_words = 3; out[k++] = P;                                 // the frame alone: no share word
    P = good(); P.lm_words = 0; out[k++] = P;
    P = good(); P.lm_words = 23; out[k++] = P;                                     // 1472 < 1536 candidates
    P = good(); P.H = 8; P.W = 16; P.lm_words = 1; out[k++] = P;                   // 128 pixels: no room for 192 header bits
    P = good(); P.B = 65535; P.H = 512; P.W = 512; P.lm_words = 1024; out[k++] = P;   // B (H/2) (W/2) past 2^31 - 1
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
    const size_t aws = codec_pee_blind_auto_workspace_bytes(&G, TM, ME);
    const size_t vws = codec_pee_blind_volume_workspace_bytes(&G, TM, ME);
    const size_t vws16 = codec_pee_blind_volume_workspace_bytes(&G, 16, ME);
    const size_t dws = codec_pee_blind_volume_workspace_bytes(&G, 1, 0);
    if (!pws || !aws || vws <= aws || vws16 <= vws || !dws || dws >= vws) {
        fprintf(stderr, "FAIL workspace sizes of good arguments: %zu / %zu / %zu / %zu / %zu\n", pws, aws, vws, vws16, dws);
        ++g_fail;
    }

#define WSB(P, tm, me) codec_pee_blind_volume_workspace_bytes(P, tm, me)
#define PLAN(P, cv, tm, nb, pol, n, off, len, sk, fr, info) \
    codec_pee_blind_volume_plan(P, cv, tm, nb, pol, 7u, 1, 9u, n, off, len, sk, fr, info, nullptr)
#define EMB(P, cover, stego, bits, nb, pol, tm, me, crc, n, off, fr, info, si, ts, m, lm, ws, wsb) \
    codec_pee_blind_volume_embed(P, cover, stego, bits, nb, pol, tm, me, 7u, 1, 9u, crc, n, off, fr, info, si, ts, m, lm, ws, wsb, nullptr)
#define ORD(P, rows, uw, hdr, sk, info, tab, ws, wsb) codec_pee_blind_volume_order(P, rows, uw, hdr, sk, info, tab, ws, wsb, nullptr)
#define GAT(P, rows, uw, info, bits, sw, ws, wsb) codec_pee_blind_volume_gather(P, rows, uw, info, bits, sw, ws, wsb, nullptr)
#define EXT(P, st, hdr, m, sk, cov, rows, uw, bits, sw, info, tab, ws, wsb) \
    codec_pee_blind_volume_extract(P, st, hdr, m, sk, cov, rows, uw, bits, sw, info, tab, ws, wsb, nullptr)

    // ---- bad parameter sets: every entry
    codec_pee_params bad[32];
    const int nbad = bad_params(bad);
    for (int k = 0; k < nbad; ++k) {
        const codec_pee_params* B = &bad[k];
        EXPECT_EQ(WSB(B, TM, ME), 0);
        EXPECT_NEG(PLAN(B, i32, TM, NB, 0, i32, i32, i32, i32, u32, i32));
        EXPECT_NEG(EMB(B, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(ORD(B, u64p, UW, u32, i32, i32, i32, p, big));
        EXPECT_NEG(GAT(B, u64p, UW, i32, u64p, 4, p, big));
        EXPECT_NEG(EXT(B, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, big));
    }
    EXPECT_EQ(WSB(nullptr, TM, ME), 0);
    EXPECT_NEG(PLAN(nullptr, i32, TM, NB, 0, i32, i32, i32, i32, u32, i32));
    EXPECT_NEG(EMB(nullptr, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, big));
    EXPECT_NEG(ORD(nullptr, u64p, UW, u32, i32, i32, i32, p, big));
    EXPECT_NEG(GAT(nullptr, u64p, UW, i32, u64p, 4, p, big));
    EXPECT_NEG(EXT(nullptr, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, big));
    for (int k = 0; k < 2; ++k) {   // H or W above 65535: the reserved rectangle travels in the ROI record words
        codec_pee_params P = good();
        P.B = 1;
        if (k == 0) { P.H = 65536; P.W = 8; } else { P.H = 8; P.W = 65536; }
        P.lm_words = (4 * 32768 + 63) / 64;
        if (!codec_pee_workspace_bytes(&P)) { fprintf(stderr, "FAIL: the tall / wide shape is not a codec_pee one\n"); ++g_fail; }
        EXPECT_EQ(WSB(&P, TM, ME), 0);
        EXPECT_NEG(EMB(&P, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, big));
        EXPECT_NEG(EXT(&P, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, big));
    }
    // ---- tmax, max_entries, nbits, policy
    for (int32_t tm : {0, -1, 17, 64, INT32_MIN, INT32_MAX}) {
        EXPECT_EQ(WSB(&G, tm, ME), 0);
        EXPECT_NEG(PLAN(&G, i32, tm, NB, 0, i32, i32, i32, i32, u32, i32));
        EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, tm, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, big));
    }
    for (int32_t me : {-1, INT32_MIN, CODEC_PEE_BLIND_MAX_ENTRIES + 1, INT32_MAX}) {
        EXPECT_EQ(WSB(&G, TM, me), 0);
        EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, me, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, big));
    }
    for (int64_t nb : {(int64_t)0, (int64_t)-1, (int64_t)1 << 31, INT64_MIN, INT64_MAX}) {
        EXPECT_NEG(PLAN(&G, i32, TM, nb, 0, i32, i32, i32, i32, u32, i32));
        EXPECT_NEG(EMB(&G, p, q, u64p, nb, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    }
    for (int32_t pol : {-1, 2, INT32_MIN, INT32_MAX}) {
        EXPECT_NEG(PLAN(&G, i32, TM, NB, pol, i32, i32, i32, i32, u32, i32));
        EXPECT_NEG(EMB(&G, p, q, u64p, NB, pol, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    }
    // ---- the plan's pointers
    EXPECT_NEG(PLAN(&G, nullptr, TM, NB, 0, i32, i32, i32, i32, u32, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, nullptr, i32, i32, i32, u32, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, i32, nullptr, i32, i32, u32, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, i32, i32, nullptr, i32, u32, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, i32, i32, i32, nullptr, u32, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, i32, i32, i32, i32, nullptr, i32));
    EXPECT_NEG(PLAN(&G, i32, TM, NB, 0, i32, i32, i32, i32, u32, nullptr));
    // ---- the embed's pointers, its own rules, the workspace
    EXPECT_NEG(EMB(&G, nullptr, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, nullptr, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, nullptr, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, nullptr, i32, u32, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, nullptr, u32, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, nullptr, i32, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, nullptr, i32, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, nullptr, i32, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, nullptr, meta, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, nullptr, u64p, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, nullptr, p, vws));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, nullptr, vws));
    EXPECT_NEG(EMB(&G, p, p, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));   // in place
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws - 1));
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, aws));   // the blind workspace: short
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, 16, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, vws));   // sized for TM, asked for 16
    EXPECT_NEG(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, p, 0));
    // ---- order, gather, extract: row and stream widths, pointers, the workspace
    for (int32_t w : {0, -1, 2, (1 << 24) + 1, INT32_MIN, INT32_MAX}) {
        EXPECT_NEG(ORD(&G, u64p, w, u32, i32, i32, i32, p, dws));
        EXPECT_NEG(GAT(&G, u64p, w, i32, u64p, 4, p, dws));
        EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, w, u64p, 4, i32, i32, p, dws));
    }
    for (int64_t sw : {(int64_t)-1, ((int64_t)1 << 25) + 1, INT64_MIN, INT64_MAX}) {
        EXPECT_NEG(GAT(&G, u64p, UW, i32, u64p, sw, p, dws));
        EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, sw, i32, i32, p, dws));
    }
    EXPECT_NEG(ORD(&G, nullptr, UW, u32, i32, i32, i32, p, dws));
    EXPECT_NEG(ORD(&G, u64p, UW, nullptr, i32, i32, i32, p, dws));
    EXPECT_NEG(ORD(&G, u64p, UW, u32, i32, nullptr, i32, p, dws));
    EXPECT_NEG(ORD(&G, u64p, UW, u32, i32, i32, nullptr, p, dws));
    EXPECT_NEG(ORD(&G, u64p, UW, u32, i32, i32, i32, nullptr, dws));
    EXPECT_NEG(ORD(&G, u64p, UW, u32, i32, i32, i32, p, dws - 1));
    EXPECT_NEG(ORD(&G, u64p, UW, u32, i32, i32, i32, p, 0));
    EXPECT_NEG(GAT(&G, nullptr, UW, i32, u64p, 4, p, dws));
    EXPECT_NEG(GAT(&G, u64p, UW, nullptr, u64p, 4, p, dws));
    EXPECT_NEG(GAT(&G, u64p, UW, i32, nullptr, 4, p, dws));
    EXPECT_NEG(GAT(&G, u64p, UW, i32, u64p, 4, nullptr, dws));
    EXPECT_NEG(GAT(&G, u64p, UW, i32, u64p, 4, p, dws - 1));
    EXPECT_NEG(EXT(&G, nullptr, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, nullptr, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, nullptr, i32, q, u64p, UW, u64p, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, nullptr, u64p, UW, u64p, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, nullptr, UW, u64p, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, nullptr, 4, i32, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, nullptr, i32, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, nullptr, p, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, nullptr, dws));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, p, u64p, UW, u64p, 4, i32, i32, p, dws));   // in place
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, dws - 1));
    EXPECT_NEG(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, p, pws));

    expect_no_device_ops();

    // ---- good arguments: each entry gets past its checks and reaches a device operation, which
    // the stubs refuse and count.  The buffers stand in for device memory: nothing dereferences
    // them on the host.
    {
        static unsigned char ws[1 << 23];
        if (vws16 > sizeof(ws)) { fprintf(stderr, "FAIL: workspace of the good shape is %zu bytes\n", vws16); return 2; }
        g_ops = hip_stub_device_ops();
        EXPECT_REACHED(PLAN(&G, i32, TM, NB, 0, i32, i32, i32, i32, u32, i32));
        EXPECT_REACHED(PLAN(&G, i32, 1, 1, 1, i32, i32, i32, i32, u32, i32));
        EXPECT_REACHED(PLAN(&G, i32, 16, 0x7FFFFFFFLL, 1, i32, i32, i32, i32, u32, i32));
        EXPECT_REACHED(EMB(&G, p, q, u64p, NB, 0, TM, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, ws, vws));
        EXPECT_REACHED(EMB(&G, p, q, u64p, NB, 1, TM, ME, nullptr, i32, i32, u32, i32, i32, i32, meta, u64p, ws, vws));   // no cover CRC
        EXPECT_REACHED(EMB(&G, buf + 2, q, u64p, 1, 0, 16, ME, u32, i32, i32, u32, i32, i32, i32, meta, u64p, ws, vws16));  // an offset view
        EXPECT_REACHED(ORD(&G, u64p, UW, u32, i32, i32, i32, ws, dws));
        EXPECT_REACHED(ORD(&G, u64p, 3, u32, nullptr, i32, i32, ws, dws));          // no skip marks: every slice a carrier
        EXPECT_REACHED(GAT(&G, u64p, UW, i32, u64p, 4, ws, dws));
        EXPECT_REACHED(EXT(&G, p, u32, meta, i32, q, u64p, UW, u64p, 4, i32, i32, ws, dws));
        EXPECT_REACHED(EXT(&G, p, u32, meta, nullptr, q, u64p, UW, nullptr, 0, i32, i32, ws, dws));   // no stream asked for
    }
    return abi_report("abi_args_blind_vol");
}

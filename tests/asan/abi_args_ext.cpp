// Host sanitizer check of the argument validation of include/codec_tcc_ext.h's entries, as
// abi_args.cpp is for codec_tcc.h: linked against the host-only -fsanitize=address,undefined
// build of the library and tests/asan/hip_stubs.cpp (tests/test_asan_abi.py builds and runs
// it on the CPU box).  Every call has NULL pointers, a bad shape, tmin / tmax out of range,
// cover == stego or a short workspace, and must return its negative status with an error text.
// No call here reaches a kernel launch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "codec_tcc_ext.h"

#include "abi_expect.h"

static codec_pee_params good_pee() {
    codec_pee_params P;
    P.B = 2; P.H = 64; P.W = 64; P.bytes = 2; P.T = 2; P.maxval = 65535; P.payload_words = 1;
    P.lm_words = (32 * 32 + 63) / 64;
    return P;
}

// every way the shape part of a codec_pee_params can be invalid (P.T is ignored by the entry)
static std::vector<codec_pee_params> bad_pee() {
    std::vector<codec_pee_params> v;
    codec_pee_params P;
    P = good_pee(); P.B = 0; v.push_back(P);
    P = good_pee(); P.B = INT32_MIN; v.push_back(P);
    P = good_pee(); P.H = 0; v.push_back(P);
    P = good_pee(); P.W = -3; v.push_back(P);
    P = good_pee(); P.H = 65536; P.W = 65536; v.push_back(P);
    P = good_pee(); P.B = INT32_MAX; P.H = 32768; P.W = 32768; v.push_back(P);   // batch too large
    P = good_pee(); P.bytes = 4; v.push_back(P);
    P = good_pee(); P.maxval = 0; v.push_back(P);
    P = good_pee(); P.maxval = 65536; v.push_back(P);
    P = good_pee(); P.bytes = 1; P.maxval = 256; v.push_back(P);
    P = good_pee(); P.payload_words = 0; v.push_back(P);
    P = good_pee(); P.lm_words = 0; v.push_back(P);
    P = good_pee(); P.lm_words = 15; v.push_back(P);                        // < nc / 64
    return v;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    alignas(64) static unsigned char buf2[1 << 16];
    void* p = buf;
    void* q = buf2;
    uint64_t* w64 = reinterpret_cast<uint64_t*>(buf);
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    codec_pee_meta* pmeta = reinterpret_cast<codec_pee_meta*>(buf);

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }
    codec_set_tuning(1);

    for (const codec_pee_params& P : bad_pee())
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, pmeta, w64, p, 1u << 30, nullptr));
    {
        const codec_pee_params P = good_pee();
        const size_t ws = codec_pee_workspace_bytes(&P);
        if (ws == 0) { fprintf(stderr, "FAIL pee workspace_bytes of good params\n"); ++g_fail; }
        EXPECT_NEG(codec_pee_multi_embed_auto(nullptr, p, q, w64, i32, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, nullptr, q, w64, i32, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, nullptr, w64, i32, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, nullptr, i32, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, nullptr, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, nullptr, pmeta, w64, p, ws, nullptr));   // t_out required
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, nullptr, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, pmeta, nullptr, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, pmeta, w64, nullptr, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, nullptr, nullptr, w64, i32, 1, 4, i32, pmeta, w64, p, ws, nullptr));
        // tmin / tmax out of range
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 0, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, -1, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 5, 4, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 65, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 0, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, INT32_MIN, INT32_MAX, i32, pmeta, w64, p, ws, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 65, 65, i32, pmeta, w64, p, ws, nullptr));
        // in place
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, p, w64, i32, 1, 4, i32, pmeta, w64, q, ws, nullptr));
        // short workspace
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, pmeta, w64, p, ws - 1, nullptr));
        EXPECT_NEG(codec_pee_multi_embed_auto(&P, p, q, w64, i32, 1, 4, i32, pmeta, w64, p, 0, nullptr));
    }
    expect_no_device_ops();
    return abi_report("abi_args_ext");
}

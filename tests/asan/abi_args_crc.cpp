// Host sanitizer check of the argument validation of include/codec_tcc_crc.h's entries, as
// abi_args_ext.cpp is for codec_tcc_ext.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status (0 for the size queries) with an error text and no device operation; the pure-host
// combine entry also runs its known answers and a split-buffer identity here.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_crc.h"

#include "abi_expect.h"

static uint32_t combine(uint32_t a, uint32_t b, uint64_t len_b) {
    uint32_t out = 0;
    if (codec_crc32_combine(a, b, len_b, &out) != 0) { ++g_fail; fprintf(stderr, "FAIL combine status\n"); }
    return out;
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }

    // ---- size queries
    const size_t chunk = codec_crc32_chunk_bytes();
    if (chunk == 0 || chunk % 16) { fprintf(stderr, "FAIL chunk bytes %zu\n", chunk); ++g_fail; }
    EXPECT_EQ(codec_crc32_workspace_bytes(0, 4, 4, 1), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(-1, 4, 4, 1), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(INT32_MIN, 4, 4, 1), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 0, 4, 1), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 4, -4, 2), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 4, 4, 0), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 4, 4, 3), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 4, 4, 4), 0);
    EXPECT_EQ(codec_crc32_workspace_bytes(1, 65536, 65536, 2), 0);                  // slice too large
    EXPECT_EQ(codec_crc32_workspace_bytes(INT32_MAX, 32768, 32768, 2), 0);          // batch too large
    const size_t ws = codec_crc32_workspace_bytes(2, 64, 64, 2);
    if (ws < 2 * 4) { fprintf(stderr, "FAIL workspace_bytes of good arguments: %zu\n", ws); ++g_fail; }
    if (codec_crc32_workspace_bytes(1, 1, (int32_t)chunk + 1, 1) < 2 * 4) { fprintf(stderr, "FAIL two chunks\n"); ++g_fail; }

    // ---- codec_crc32_slices: every bad argument is refused before any device operation
    EXPECT_NEG(codec_crc32_slices(0, 64, 64, 2, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(-2, 64, 64, 2, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(INT32_MIN, 64, 64, 2, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 0, 64, 2, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, -1, 2, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 0, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 3, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 4, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, -1, p, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, nullptr, u32, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, p, nullptr, p, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, p, u32, nullptr, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, nullptr, nullptr, nullptr, ws, nullptr));
    EXPECT_NEG(codec_crc32_slices(1, 65536, 65536, 1, p, u32, p, 1u << 30, nullptr));          // slice too large
    EXPECT_NEG(codec_crc32_slices(1, INT32_MAX, INT32_MAX, 2, p, u32, p, 1u << 30, nullptr));
    EXPECT_NEG(codec_crc32_slices(INT32_MAX, 32768, 32768, 2, p, u32, p, 1u << 30, nullptr));  // batch too large
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, p, u32, p, ws - 1, nullptr));                  // short workspace
    EXPECT_NEG(codec_crc32_slices(2, 64, 64, 2, p, u32, p, 0, nullptr));
    EXPECT_NEG(codec_crc32_slices(1, 1, (int32_t)chunk + 1, 1, p, u32, p, 4, nullptr));        // two chunks need 8

    // ---- codec_crc32_combine (pure host)
    EXPECT_NEG(codec_crc32_combine(1, 2, 3, nullptr));
    EXPECT_EQ(combine(0x9BE3E0A3u, 0x131DA070u, 5), 0xCBF43926u);   // "1234" || "56789"
    EXPECT_EQ(combine(0x9BE3E0A3u, 0u, 0), 0x9BE3E0A3u);            // B empty: crc(B) = 0
    EXPECT_EQ(combine(0u, 0x131DA070u, 5), 0x131DA070u);            // A empty
    EXPECT_EQ(combine(0x83DCEFB7u, 0x4F5344CDu, 1), 0x4F5344CDu ^ combine(0x83DCEFB7u, 0u, 1));   // linear in crc_b
    // associative: ("1234" || "56") || "789" = "1234" || ("56" || "789")
    {
        const uint32_t c1234 = 0x9BE3E0A3u;
        const uint32_t c56789 = 0x131DA070u;
        for (uint64_t n : {0ull, 1ull, 3ull, 1ull << 20, (1ull << 32) + 3, ~0ull}) {
            const uint32_t left = combine(combine(c1234, c56789, 5), 0x12345678u, n);
            const uint32_t right = combine(c1234, combine(c56789, 0x12345678u, n), 5 + n);
            if (n != ~0ull) EXPECT_EQ(left, right);   // 5 + n wraps for the last one: only run it
        }
        // x has order 2^32 - 1: a shift by 2^32 + 3 bytes is a shift by 4
        EXPECT_EQ(combine(c1234, 0u, (1ull << 32) + 3), combine(c1234, 0u, 4));
    }

    expect_no_device_ops();
    return abi_report("abi_args_crc");
}

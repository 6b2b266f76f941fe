// Host sanitizer check of the argument validation of include/codec_tcc_aead.h's entries, as
// abi_args_crc.cpp is for codec_tcc_crc.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status (0 for the size queries) with an error text and no device operation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_aead.h"

#include "abi_expect.h"

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    const codec_aead_ctx* ctx = reinterpret_cast<const codec_aead_ctx*>(buf);
    uint64_t* rows = reinterpret_cast<uint64_t*>(buf);
    int32_t* len = reinterpret_cast<int32_t*>(buf);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    const uint32_t STREAM = CODEC_AEAD_STREAM_INDEX;
    const size_t big = (size_t)1 << 30;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }
    if (sizeof(codec_aead_ctx) != 48) { fprintf(stderr, "FAIL ctx size %zu\n", sizeof(codec_aead_ctx)); ++g_fail; }

    // ---- size queries
    const size_t chunk = codec_poly1305_chunk_bytes();
    if (chunk == 0 || chunk % 16) { fprintf(stderr, "FAIL chunk bytes %zu\n", chunk); ++g_fail; }
    EXPECT_EQ(codec_aead_workspace_bytes(0, 16, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(-1, 16, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(INT32_MIN, 16, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, -1, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, INT64_MIN, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, INT64_MAX, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, (1ll << 32) + 1, 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, 16, -1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(1, 16, CODEC_AEAD_MAX_ROW_WORDS + 1), 0);
    EXPECT_EQ(codec_aead_workspace_bytes(INT32_MAX, 1ll << 32, 1), 0);   // batch too large
    const size_t ws = codec_aead_workspace_bytes(2, 100, 4);
    const size_t ws0 = codec_aead_workspace_bytes(2, 0, 0);
    if (ws == 0 || ws0 == 0 || ws < ws0 || ws > sizeof(buf)) { fprintf(stderr, "FAIL workspace_bytes %zu %zu\n", ws, ws0); ++g_fail; }
    if (codec_aead_workspace_bytes(1, (int64_t)chunk * 64, 0) <= codec_aead_workspace_bytes(1, (int64_t)chunk, 0)) {
        fprintf(stderr, "FAIL workspace does not grow with the chunks\n"); ++g_fail;
    }

    // ---- codec_chacha20_rows
    EXPECT_NEG(codec_chacha20_rows(ctx, 0, 0, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, -3, 0, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, INT32_MIN, 0, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, 0, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, -1, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, CODEC_AEAD_MAX_ROW_WORDS + 1, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, INT32_MAX, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, INT32_MAX, 0, rows, CODEC_AEAD_MAX_ROW_WORDS, len, rows, nullptr));   // batch too large
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0x7FFFFFFFu, rows, 4, len, rows, nullptr));    // the second index is 2^31
    EXPECT_NEG(codec_chacha20_rows(ctx, 1, STREAM + 1, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, STREAM, rows, 4, len, rows, nullptr));          // the stream is one row
    EXPECT_NEG(codec_chacha20_rows(ctx, 1, 0xFFFFFFFFu, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(nullptr, 2, 0, rows, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, nullptr, 4, len, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, 4, nullptr, rows, nullptr));
    EXPECT_NEG(codec_chacha20_rows(ctx, 2, 0, rows, 4, len, nullptr, nullptr));
    EXPECT_NEG(codec_chacha20_rows(nullptr, 1, STREAM, nullptr, 4, nullptr, nullptr, nullptr));

    // ---- codec_poly1305_tags
    EXPECT_NEG(codec_poly1305_tags(ctx, 0, 0, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, -1, 0, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, -1, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, INT64_MIN, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, INT64_MAX, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, nullptr, 100, rows, 4, len, u32, p, big, nullptr));   // bytes without a pointer
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 0, rows, 4, len, u32, p, big, nullptr));           // a pointer without bytes
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 0, len, u32, p, big, nullptr));         // row_words 0 with rows
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 0, nullptr, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, nullptr, 0, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, -4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, CODEC_AEAD_MAX_ROW_WORDS + 1, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, nullptr, 4, len, u32, p, big, nullptr));      // rows without lengths and back
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 4, nullptr, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, INT32_MAX, 0, p, 1ll << 32, rows, 4, len, u32, p, big, nullptr));   // batch too large
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0x7FFFFFFFu, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, STREAM, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(nullptr, 2, 0, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 4, len, nullptr, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 4, len, u32, nullptr, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 4, len, u32, p, ws - 1, nullptr));      // short workspace
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, p, 100, rows, 4, len, u32, p, 0, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 2, 0, nullptr, 0, nullptr, 0, nullptr, u32, p, ws0 - 1, nullptr));
    EXPECT_NEG(codec_poly1305_tags(ctx, 1, 0, p, (int64_t)chunk * 4, nullptr, 0, nullptr, u32, p,
                                   codec_aead_workspace_bytes(1, (int64_t)chunk * 4, 0) - 1, nullptr));

    // ---- codec_poly1305_tags_otk
    EXPECT_NEG(codec_poly1305_tags_otk(nullptr, 2, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 0, p, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, p, -100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, nullptr, 100, rows, 4, len, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, p, 100, rows, 4, nullptr, u32, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, p, 100, rows, 4, len, nullptr, p, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, p, 100, rows, 4, len, u32, nullptr, big, nullptr));
    EXPECT_NEG(codec_poly1305_tags_otk(u32, 2, p, 100, rows, 4, len, u32, p, ws - 1, nullptr));

    // ---- codec_aead_release
    EXPECT_NEG(codec_aead_release(ctx, 0, 0, u32, u32, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, rows, 0, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, rows, CODEC_AEAD_MAX_ROW_WORDS + 1, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0x7FFFFFFFu, u32, u32, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, STREAM, u32, u32, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(nullptr, 2, 0, u32, u32, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, nullptr, u32, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, nullptr, rows, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, nullptr, 4, len, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, rows, 4, nullptr, rows, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, rows, 4, len, nullptr, len, nullptr));
    EXPECT_NEG(codec_aead_release(ctx, 2, 0, u32, u32, rows, 4, len, rows, nullptr, nullptr));

    expect_no_device_ops();
    return abi_report("abi_args_aead");
}

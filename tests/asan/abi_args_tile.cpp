// Host sanitizer check of the argument validation of include/codec_tcc_tile.h's entries, as
// abi_args_crc.cpp is for codec_tcc_crc.h: linked against the host-only
// -fsanitize=address,undefined build of the library and tests/asan/hip_stubs.cpp
// (tests/test_asan_abi.py builds and runs it).  Every bad call must return its negative
// status with an error text and no device operation; the two pure-host entries (grid, route)
// also run their good cases here.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "codec_tcc_tile.h"

#include "abi_expect.h"

static void expect_grid(int32_t H, int32_t W, int32_t th, int32_t tw, int32_t wy, int32_t wx) {
    int32_t ny = -1, nx = -1;
    EXPECT_EQ(codec_crc32_tiles_grid(H, W, th, tw, &ny, &nx), 0);
    EXPECT_EQ(ny, wy);
    EXPECT_EQ(nx, wx);
}

int main() {
    alignas(64) static unsigned char buf[1 << 16];
    void* p = buf;
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    uint64_t* u64p = reinterpret_cast<uint64_t*>(buf);
    int32_t* i32 = reinterpret_cast<int32_t*>(buf);
    int32_t ny = -7, nx = -7;

    if (codec_abi_version() != 1) { fprintf(stderr, "FAIL abi version\n"); return 2; }

    // ---- codec_crc32_tiles_grid (pure host)
    expect_grid(64, 128, 64, 64, 1, 2);
    expect_grid(37, 53, 8, 8, 5, 7);
    expect_grid(37, 53, 64, 64, 1, 1);          // a tile larger than the image
    expect_grid(130, 192, 64, 64, 3, 3);
    expect_grid(1, 1, 4, 4, 1, 1);
    expect_grid(2048, 2048, 4, 4, 512, 512);
    expect_grid(2048, 2048, 1024, 1024, 2, 2);
    expect_grid(1025, 1023, 1024, 1024, 2, 1);
    expect_grid(1, INT32_MAX, 4, 1024, 1, 1 << 21);
    expect_grid(INT32_MAX, 1, 4, 4, 1 << 29, 1);
    expect_grid(32768, 65536, 1024, 4, 32, 16384);   // H * W = 2^31 exactly: allowed
    for (int32_t bad : {3, 0, -1, -64, 1025, 4096, INT32_MAX, INT32_MIN}) {
        EXPECT_NEG(codec_crc32_tiles_grid(64, 64, bad, 8, &ny, &nx));
        EXPECT_NEG(codec_crc32_tiles_grid(64, 64, 8, bad, &ny, &nx));
        EXPECT_NEG(codec_crc32_tiles_grid(64, 64, bad, bad, &ny, &nx));
    }
    for (int32_t bad : {0, -1, INT32_MIN}) {
        EXPECT_NEG(codec_crc32_tiles_grid(bad, 64, 8, 8, &ny, &nx));
        EXPECT_NEG(codec_crc32_tiles_grid(64, bad, 8, 8, &ny, &nx));
    }
    EXPECT_NEG(codec_crc32_tiles_grid(65536, 65536, 8, 8, &ny, &nx));          // slice too large
    EXPECT_NEG(codec_crc32_tiles_grid(32768, 65537, 8, 8, &ny, &nx));
    EXPECT_NEG(codec_crc32_tiles_grid(INT32_MAX, INT32_MAX, 1024, 1024, &ny, &nx));
    EXPECT_NEG(codec_crc32_tiles_grid(64, 64, 8, 8, nullptr, &nx));
    EXPECT_NEG(codec_crc32_tiles_grid(64, 64, 8, 8, &ny, nullptr));
    EXPECT_NEG(codec_crc32_tiles_grid(64, 64, 8, 8, nullptr, nullptr));
    EXPECT_EQ(ny, -7);   // a refused call writes nothing
    EXPECT_EQ(nx, -7);

    // ---- codec_crc32_tiles_route (pure host; the pointer is looked at, never read)
    EXPECT_EQ(codec_crc32_tiles_route(3, 64, 128, 2, 64, 64, p), CODEC_TILE_ROUTE_VECTOR);
    EXPECT_EQ(codec_crc32_tiles_route(3, 64, 128, 2, 16, 8, p), CODEC_TILE_ROUTE_VECTOR);
    EXPECT_EQ(codec_crc32_tiles_route(3, 64, 128, 2, 8, 4, p), CODEC_TILE_ROUTE_BYTES);
    EXPECT_EQ(codec_crc32_tiles_route(2, 37, 53, 2, 8, 8, p), CODEC_TILE_ROUTE_BYTES);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 136, 2, 64, 64, p), CODEC_TILE_ROUTE_VECTOR);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 132, 2, 64, 64, p), CODEC_TILE_ROUTE_BYTES);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 128, 1, 64, 64, p), CODEC_TILE_ROUTE_VECTOR);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 128, 1, 8, 8, p), CODEC_TILE_ROUTE_BYTES);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 128, 2, 64, 64, buf + 1), CODEC_TILE_ROUTE_BYTES);
    EXPECT_EQ(codec_crc32_tiles_route(2, 64, 128, 2, 64, 64, buf + 16), CODEC_TILE_ROUTE_VECTOR);
    EXPECT_EQ(codec_crc32_tiles_route(1, 32768, 65536, 2, 1024, 1024, p), CODEC_TILE_ROUTE_VECTOR);

    // ---- the argument rules codec_crc32_tiles_route and codec_crc32_tiles share
    struct { int32_t B, H, W, bytes, th, tw; } bad[] = {
        {0, 64, 64, 2, 8, 8},        {-2, 64, 64, 2, 8, 8},         {INT32_MIN, 64, 64, 2, 8, 8},
        {2, 0, 64, 2, 8, 8},         {2, 64, -1, 2, 8, 8},          {2, INT32_MIN, 64, 2, 8, 8},
        {2, 64, 64, 0, 8, 8},        {2, 64, 64, 3, 8, 8},          {2, 64, 64, 4, 8, 8},
        {2, 64, 64, -1, 8, 8},       {2, 64, 64, 2, 3, 8},          {2, 64, 64, 2, 8, 3},
        {2, 64, 64, 2, 0, 0},        {2, 64, 64, 2, -8, 8},         {2, 64, 64, 2, 1025, 8},
        {2, 64, 64, 2, 8, 1025},     {2, 64, 64, 2, INT32_MAX, 8},  {2, 64, 64, 2, 8, INT32_MIN},
        {1, 65536, 65536, 1, 8, 8},  {1, INT32_MAX, INT32_MAX, 2, 1024, 1024},   // slice too large
        {INT32_MAX, 64, 64, 2, 4, 4},                                             // B * nty * ntx >= 2^31
        {1 << 23, 64, 64, 1, 4, 4},                                               // = 2^31 exactly
        {16, 32768, 65536, 1, 4, 4},                                              // 16 slices of 2^27 tiles
    };
    for (const auto& a : bad) {
        EXPECT_NEG(codec_crc32_tiles_route(a.B, a.H, a.W, a.bytes, a.th, a.tw, p));
        EXPECT_NEG(codec_crc32_tiles(a.B, a.H, a.W, a.bytes, a.th, a.tw, p, u32, nullptr));
    }
    EXPECT_NEG(codec_crc32_tiles_route(2, 64, 64, 2, 8, 8, nullptr));
    EXPECT_NEG(codec_crc32_tiles(2, 64, 64, 2, 8, 8, nullptr, u32, nullptr));
    EXPECT_NEG(codec_crc32_tiles(2, 64, 64, 2, 8, 8, p, nullptr, nullptr));
    EXPECT_NEG(codec_crc32_tiles(2, 64, 64, 2, 8, 8, nullptr, nullptr, nullptr));
    EXPECT_NEG(codec_crc32_tiles(2, 64, 64, 1, 64, 64, nullptr, u32, nullptr));

    // ---- codec_crc32_tiles_compare
    EXPECT_NEG(codec_crc32_tiles_compare(0, 8, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(-1, 8, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(INT32_MIN, 8, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 0, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, -5, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, INT32_MIN, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 1 << 30, u32, u32, u64p, i32, nullptr));          // = 2^31
    EXPECT_NEG(codec_crc32_tiles_compare(INT32_MAX, INT32_MAX, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(INT32_MAX, 2, u32, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 8, nullptr, u32, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 8, u32, nullptr, u64p, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 8, u32, u32, nullptr, i32, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 8, u32, u32, u64p, nullptr, nullptr));
    EXPECT_NEG(codec_crc32_tiles_compare(2, 8, nullptr, nullptr, nullptr, nullptr, nullptr));

    expect_no_device_ops();
    return abi_report("abi_args_tile");
}

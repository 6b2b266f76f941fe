// abi_expect.h -- the expectations, counters and closing report the C-ABI drivers abi_args*.cpp
// share.  A driver is a stand-alone program linked against the host-only sanitizer build of the
// library and tests/asan/hip_stubs.cpp (tests/asan_build.py); tests/test_asan_abi.py runs it.
#pragma once
#include <stdio.h>

#include "codec_tcc.h"

static int g_fail = 0, g_n = 0;
[[maybe_unused]] static int g_ops = 0;      // device operations counted so far (EXPECT_REACHED)
extern "C" int hip_stub_device_ops(void);   // tests/asan/hip_stubs.cpp

// a negative status AND an error text
#define EXPECT_NEG(expr)                                                                           \
    do {                                                                                           \
        ++g_n;                                                                                     \
        const long long r_ = (long long)(expr);                                                    \
        if (r_ >= 0) {                                                                             \
            fprintf(stderr, "FAIL line %d: %s returned %lld (want < 0)\n", __LINE__, #expr, r_);   \
            ++g_fail;                                                                              \
        } else if (!codec_last_error() || !codec_last_error()[0]) {                                \
            fprintf(stderr, "FAIL line %d: %s gave no error message\n", __LINE__, #expr);          \
            ++g_fail;                                                                              \
        }                                                                                          \
    } while (0)

#define EXPECT_ZERO(expr)                                                                          \
    do {                                                                                           \
        ++g_n;                                                                                     \
        const long long r_ = (long long)(expr);                                                    \
        if (r_ != 0) {                                                                             \
            fprintf(stderr, "FAIL line %d: %s returned %lld (want 0)\n", __LINE__, #expr, r_);     \
            ++g_fail;                                                                              \
        }                                                                                          \
    } while (0)

#define EXPECT_EQ(expr, want)                                                                      \
    do {                                                                                           \
        ++g_n;                                                                                     \
        const unsigned long long r_ = (unsigned long long)(expr), w_ = (unsigned long long)(want); \
        if (r_ != w_) {                                                                            \
            fprintf(stderr, "FAIL line %d: %s = %llu (want %llu)\n", __LINE__, #expr, r_, w_);     \
            ++g_fail;                                                                              \
        }                                                                                          \
    } while (0)

// good arguments: the entry gets past its checks and reaches a device operation, which the
// stubs refuse and count (set g_ops = hip_stub_device_ops() before the first one)
#define EXPECT_REACHED(expr)                                                                       \
    do {                                                                                           \
        ++g_n;                                                                                     \
        (void)(expr);   /* whatever the refused launches make of it */                             \
        if (hip_stub_device_ops() <= g_ops) {                                                      \
            fprintf(stderr, "FAIL line %d: %s stopped before any device operation: %s\n", __LINE__, #expr, codec_last_error()); \
            ++g_fail;                                                                              \
        }                                                                                          \
        g_ops = hip_stub_device_ops();                                                             \
    } while (0)

// after the argument-error calls: none of them may have reached the runtime
static inline void expect_no_device_ops(void) {
    if (hip_stub_device_ops() != 0) {
        fprintf(stderr, "FAIL: %d device operations were attempted by argument-error calls\n", hip_stub_device_ops());
        ++g_fail;
    }
}

// the closing report line tests/test_asan_abi.py reads; main's return value
static inline int abi_report(const char* driver) {
    printf("%s: %d calls, %d failures\n", driver, g_n, g_fail);
    return g_fail ? 1 : 0;
}

/* What every *_errors.c checker of this directory starts from: the counters, EXPECT / EXPECT_RC,
 * fake device pointers and the final report.  Each checker is one translation unit with its own
 * main(), built by tests/c_checker.py against the product library and by csrc/Makefile
 * `check-asan` under host AddressSanitizer. */
#ifndef LDM_TESTS_C_CHECK_H
#define LDM_TESTS_C_CHECK_H
#include <stdint.h>
#include <stdio.h>

#include "ldm_sdf.h"

static int fails = 0, checks = 0;
#define EXPECT(cond)                                                               \
    do {                                                                           \
        ++checks;                                                                  \
        if (!(cond)) {                                                             \
            ++fails;                                                               \
            fprintf(stderr, "FAIL %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, \
                    #cond, ldm_last_error());                                      \
        }                                                                          \
    } while (0)
#define EXPECT_RC(expr, code)                                                     \
    do {                                                                          \
        const int rc_ = (expr);                                                   \
        EXPECT(rc_ == (code));                                                    \
        EXPECT(ldm_last_error() != NULL && ldm_last_error()[0] != 0);             \
    } while (0)

static uintptr_t fake_next = 0x7f0000000000ull;
/* distinct, 4 KiB aligned, never dereferenced by host code */
static inline void* fake(void) {
    fake_next += 0x1000000;
    return (void*)fake_next;
}
static inline void* off(const void* p, int bytes) {
    return (void*)((uintptr_t)p + (uintptr_t)bytes);
}

/* the last statement of main(): `return check_report("band_errors");` */
static inline int check_report(const char* name) {
    printf("%s: %d checks, %d failures\n", name, checks, fails);
    return fails ? 1 : 0;
}
#endif

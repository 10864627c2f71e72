// The one CHECK of the stand-alone host programs in this directory (tests/host_program.py builds and runs them): a broken invariant prints
// "FAILED file:line condition -- message" and is counted; main ends with `return check_summary();`, which prints "ok: 0 failed checks"
// when nothing failed and makes the exit status say the same.
#ifndef TAV_TESTS_HOST_CHECK_H
#define TAV_TESTS_HOST_CHECK_H
#include <cstdio>

static int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++failures;                                                   \
            std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                     \
            std::printf("\n");                                            \
        }                                                                 \
    } while (0)

static int check_summary() {
    std::printf("%s: %d failed checks\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
#endif

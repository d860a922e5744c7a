// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// What the stand-alone AddressSanitizer / UBSan programs of this directory (*_main.cpp) share: the CPU harness, included whole — every
// program sees the whole ABI —, and four helpers.  Each program has a main of its own and is built and run by one line, NAME being
// act_eval, batch, capacity, replay, traj or wrap:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -o NAME_asan tests/sanitizers/NAME_main.cpp && \
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ./NAME_asan
// (detect_leaks=0 as in run.sh: the harness keeps its RNG tables for the life of the process.)
#include "../cpu_harness/harness.cpp"

#include <cstdio>

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_) { fprintf(stderr, "%s: rc %d: %s\n", #call, rc_, tetris_last_error()); return 1; } \
    } while (0)
// one call with one bad argument per shared rule of this area (drl-tetris_amd/csrc/tetris_host.h): refused, nothing touched
#define REFUSED(call) \
    do { if ((call) != TETRIS_E_ARG) { fprintf(stderr, "%s: not refused\n", #call); return 1; } } while (0)
#define OK(call) \
    do { if ((call) != TETRIS_OK) { fprintf(stderr, "%s: %s\n", #call, tetris_last_error()); return 1; } } while (0)

// TEST INFRASTRUCTURE: what every sanitized driver of this directory starts and ends with, and the helpers that more
// than one of them defined in the same words.  Each driver is one translation unit with its own main.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "qsv.h"

// hip_stub.cpp
extern "C" unsigned long qsv_stub_launches;
extern "C" unsigned long qsv_stub_bytes_copied;
extern "C" int qsv_stub_devices;  // 1; a driver sets 2 while it needs a register on a second device

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: expectation failed: %s (last error: %s)\n", __FILE__, __LINE__, #cond, qsv_last_error()); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

// the summary line tests/test_sanitized_host.py reads, and main's exit status
inline int finish(const char *name) {
    std::printf("sanitized %s driver: %lu kernel launches prepared, %d failed expectations\n", name, qsv_stub_launches, failures);
    return failures ? 1 : 0;
}

struct Stats {
    uint64_t queued = 0, launched = 0;
};
inline Stats stats_of(qsv_state *st) {
    Stats s;
    EXPECT(qsv_defer_stats(st, &s.queued, &s.launched) == QSV_OK);
    return s;
}

// Kraus operators of the channel and ensemble drivers: exactly as many doubles as the call may read
inline std::vector<double> amplitude_damping(double gamma) {
    return {1, 0, 0, 0, 0, 0, std::sqrt(1 - gamma), 0, /* K1 */ 0, 0, std::sqrt(gamma), 0, 0, 0, 0, 0};
}
inline std::vector<double> bit_flip(double p) {
    return {std::sqrt(1 - p), 0, 0, 0, 0, 0, std::sqrt(1 - p), 0, /* K1 */ 0, 0, std::sqrt(p), 0, std::sqrt(p), 0, 0, 0};
}
// `count` operators on k qubits, each a multiple of a diagonal matrix that is not a multiple of the identity
inline std::vector<double> general(int k, int count) {
    const int D = 1 << k;
    std::vector<double> out(static_cast<size_t>(2) * D * D * count, 0.0);
    for (int j = 0; j < count; ++j)
        for (int r = 0; r < D; ++r) out[2 * (static_cast<size_t>(D) * D * j + r * D + r)] = std::sqrt((1.0 + r) / ((1.0 + D) * count));
    return out;
}

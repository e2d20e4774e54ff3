// TEST INFRASTRUCTURE: drives the host side of the measurement and feed-forward entry points of a trajectory ensemble
// (qsv_ensemble_measure, qsv_ensemble_apply_conditional, qsv_ensemble_bits_read, qsv_ensemble_bits_write) under ASan + UBSan
// against hip_stub.cpp (device memory is zeroed host memory and kernels do not run, so every outcome "chosen on the device"
// reads back as (0, 0.0) and the classical bits hold what was written to them from the host).
// Walks: every refusal -- null pointers, a member size out of range, qubits outside a member or repeated, a draw outside
// [0, 1) or a forced outcome outside -1 .. 1 in any member, a bit outside -1 .. 63, `after` outside 0 .. 1, k outside 1 .. 2,
// masks that share a bit, mode registers, views -- on plain and on deferring registers, each before any launch and with the
// deferred queue left as it was.  Valid calls for members of 1 to 16 qubits x 1 to 64 members on every target bit and pair:
// three launches per measurement (read pass, select, update pass), one per conditional gate, the kernel names.  The bits
// allocation made by a read before any measurement; a member-size change with and without a pending log; a log of 300 steps,
// more than its device slots, of measurements and channels mixed; destroy with everything allocated (the leak check of this
// program says so).
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "driver_common.h"

constexpr int MEASURE_LAUNCHES = 3;         // read pass, select, update pass
constexpr int CONDITIONAL_LAUNCHES = 1;
constexpr int GENERAL_LAUNCHES = 3;         // a general channel call

static const double Z0[4] = {1, 0, 0, 0}, Z1[4] = {0, 0, 1, 0};
static const double R = 0.70710678118654752440;
static const double Y0[4] = {R, 0, 0, R}, Y1[4] = {0, R, R, 0};      // complex eigenvectors
static const double H[8] = {R, 0, R, 0, R, 0, -R, 0};
static const double CX[32] = {1, 0, 0, 0, 0, 0, 0, 0, /**/ 0, 0, 1, 0, 0, 0, 0, 0, /**/ 0, 0, 0, 0, 0, 0, 1, 0, /**/ 0, 0, 0, 0, 1, 0, 0, 0};

// every refusal on a register of n + b qubits read as 2^b members of n >= 2 qubits; nothing may be launched, logged or flushed
static void call_refusals(qsv_state *st, int n, int b, qsv_state *modes, qsv_state *view) {
    const unsigned long before = qsv_stub_launches;
    const Stats was = stats_of(st);
    uint64_t steps_before = 99, steps_after = 98;
    EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps_before) == QSV_OK);
    const size_t members = size_t(1) << b;
    const std::vector<double> u(members, 0.5);
    std::vector<double> bad_u = u;
    std::vector<int> forced(members, -1);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // ---- measure
    EXPECT(qsv_ensemble_measure(nullptr, n, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n, 0, nullptr, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n, 0, Z0, nullptr, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, 0, 0, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, 0, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, -1, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n + b + 1, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n, -1, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(st, n, n, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);              // a qubit of the register, not of a member
    if (b > 0) EXPECT(qsv_ensemble_measure(st, n, n + b - 1, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    for (double wrong : {1.0, -0.1, nan, 2.0}) {                                                        // in the last member only
        bad_u.back() = wrong;
        EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, 0, 0, bad_u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, 0, 0, bad_u.data(), forced.data()) == QSV_EINVAL);
    }
    for (int wrong : {-2, 2, 99}) {
        forced.back() = wrong;
        EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, 0, 0, u.data(), forced.data()) == QSV_EINVAL);
    }
    forced.back() = -1;
    for (int wrong : {-2, 64, 1000}) EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, 0, wrong, u.data(), nullptr) == QSV_EINVAL);
    for (int wrong : {-1, 2}) EXPECT(qsv_ensemble_measure(st, n, 0, Z0, Z1, wrong, 0, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_measure(modes, 1, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_ESTATE);
    EXPECT(qsv_ensemble_measure(view, 2, 0, Z0, Z1, 0, 0, u.data(), nullptr) == QSV_EINVAL);
    // ---- conditional gates
    const int q0[2] = {0, 1}, twice[2] = {0, 0}, outside[2] = {0, n}, low[2] = {-1, 0};
    EXPECT(qsv_ensemble_apply_conditional(nullptr, n, 1, q0, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, nullptr, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, q0, nullptr, 0, 0) == QSV_EINVAL);
    for (int wrong : {0, -1, 3}) EXPECT(qsv_ensemble_apply_conditional(st, n, wrong, q0, CX, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, 0, 1, q0, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, 1, 2, q0, CX, 0, 0) == QSV_EINVAL);                         // members smaller than the gate
    EXPECT(qsv_ensemble_apply_conditional(st, n + b + 1, 1, q0, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 2, twice, CX, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 2, outside, CX, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, low, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, outside + 1, H, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, q0, H, 1, 1) == QSV_EINVAL);                          // a bit asked to be set and clear
    EXPECT(qsv_ensemble_apply_conditional(st, n, 1, q0, H, 0x8000000000000001ull, 0x8000000000000000ull) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_conditional(modes, 1, 1, q0, H, 0, 0) == QSV_ESTATE);
    EXPECT(qsv_ensemble_apply_conditional(view, 2, 1, q0, H, 0, 0) == QSV_EINVAL);
    // ---- the bits
    std::vector<uint64_t> words(members, 7);
    EXPECT(qsv_ensemble_bits_read(nullptr, n, words.data()) == QSV_EINVAL && qsv_ensemble_bits_read(st, n, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_bits_read(st, -1, words.data()) == QSV_EINVAL && qsv_ensemble_bits_read(st, n + b + 1, words.data()) == QSV_EINVAL);
    EXPECT(qsv_ensemble_bits_read(modes, 1, words.data()) == QSV_ESTATE && qsv_ensemble_bits_read(view, 2, words.data()) == QSV_EINVAL);
    EXPECT(qsv_ensemble_bits_write(nullptr, n, words.data()) == QSV_EINVAL);
    EXPECT(qsv_ensemble_bits_write(st, -1, words.data()) == QSV_EINVAL && qsv_ensemble_bits_write(st, n + b + 1, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_bits_write(modes, 1, words.data()) == QSV_ESTATE && qsv_ensemble_bits_write(view, 2, nullptr) == QSV_EINVAL);
    EXPECT(words[0] == 7 && words.back() == 7);
    const Stats now = stats_of(st);
    EXPECT(now.queued == was.queued && now.launched == was.launched);
    EXPECT(qsv_stub_launches == before);
    EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps_after) == QSV_OK && steps_after == steps_before);
}

int main() {
    qsv_state *modes = nullptr, *view = nullptr;
    EXPECT(qsv_create_qudit(2, 3, 0, &modes) == QSV_OK);
    void *view_memory = std::calloc(16, 16);
    EXPECT(qsv_create_view(4, 0, view_memory, 16, nullptr, &view) == QSV_OK);
    qsv_channel *one = nullptr, *mixed = nullptr;
    EXPECT(qsv_channel_create(1, 2, amplitude_damping(0.3).data(), 0, &one) == QSV_OK);
    EXPECT(qsv_channel_create(1, 2, bit_flip(0.25).data(), 0, &mixed) == QSV_OK);

    // ---- members of 1 to 16 qubits x 1 to 64 members: refusals, then valid calls on every target bit and pair ---------------------
    for (int n = 1; n <= 16; ++n)
        for (int b = 0; b <= 6; ++b) {
            qsv_state *st = nullptr;
            const size_t members = size_t(1) << b;
            EXPECT(qsv_create(n + b, 0, &st) == QSV_OK);
            EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 0) == QSV_OK);
            if (n >= 2) call_refusals(st, n, b, modes, view);
            // the bits exist before any measurement: a read makes them, zeroed
            std::vector<uint64_t> words(members, 7), pattern(members);
            EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words[0] == 0 && words.back() == 0);
            for (size_t m = 0; m < members; ++m) pattern[m] = 0x8000000000000001ull * (m & 1) + (m << 8);
            EXPECT(qsv_ensemble_bits_write(st, n, pattern.data()) == QSV_OK && qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words == pattern);
            std::vector<double> u(members);
            std::vector<int> forced(members);
            for (size_t m = 0; m < members; ++m) {
                u[m] = (m + 0.5) / members;
                forced[m] = static_cast<int>(m % 3) - 1;
            }
            char name[128] = "", want[128];
            uint64_t logged = 0;
            for (int cap : {0, 2}) {
                EXPECT(qsv_set_option(st, QSV_OPT_GRID_CAP, cap) == QSV_OK);
                for (int variant : {0, 1}) {
                    if (variant == 1 && (cap != 0 || (b != 0 && b != 3))) continue;
                    EXPECT(qsv_set_option(st, QSV_OPT_READOUT_VARIANT, variant) == QSV_OK);
                    for (int q = 0; q < n; ++q) {
                        const bool lane = n >= 6 && variant == 0 && n - 1 - q < 6;
                        unsigned long before = qsv_stub_launches;
                        EXPECT(qsv_ensemble_measure(st, n, q, Z0, Z1, 0, q % 64, u.data(), nullptr) == QSV_OK && qsv_stub_launches - before == MEASURE_LAUNCHES);
                        EXPECT(qsv_ensemble_measure(st, n, q, Y0, Y1, 1, -1, u.data(), forced.data()) == QSV_OK && qsv_stub_launches - before == 2 * MEASURE_LAUNCHES);
                        EXPECT(qsv_ensemble_measure(st, n, q, Y0, Y1, 0, 63, u.data(), forced.data()) == QSV_OK && qsv_stub_launches - before == 3 * MEASURE_LAUNCHES);
                        logged += 3;
                        std::snprintf(want, sizeof(want), "k_ens_channel_apply<1, %d, true> after k_ens_measure_select after k_ens_channel_rdm", lane ? 1 : 0);
                        EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        before = qsv_stub_launches;
                        EXPECT(qsv_ensemble_apply_conditional(st, n, 1, &q, H, 0, 0) == QSV_OK && qsv_stub_launches - before == CONDITIONAL_LAUNCHES);
                        EXPECT(qsv_ensemble_apply_conditional(st, n, 1, &q, H, 1ull << 63, 1) == QSV_OK && qsv_stub_launches - before == 2 * CONDITIONAL_LAUNCHES);
                        std::snprintf(want, sizeof(want), "k_ens_apply_conditional<1, %d, true>", lane ? 1 : 0);
                        EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                    }
                    for (int q0 = 0; q0 < n; ++q0)
                        for (int q1 = 0; q1 < n; ++q1) {
                            if (q0 == q1 || (n > 8 && (q0 * 7 + q1 * 3 + n + b) % 5)) continue;     // a fifth of the pairs of the larger members
                            const int qs[2] = {q0, q1};
                            const unsigned long before = qsv_stub_launches;
                            EXPECT(qsv_ensemble_apply_conditional(st, n, 2, qs, CX, 2, 1ull << 40) == QSV_OK && qsv_stub_launches - before == CONDITIONAL_LAUNCHES);
                            const int lanes = n >= 6 && variant == 0 ? (n - 1 - q0 < 6) + (n - 1 - q1 < 6) : 0;
                            std::snprintf(want, sizeof(want), "k_ens_apply_conditional<2, %d, true>", lanes);
                            EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        }
                }
            }
            uint64_t steps = 0;
            EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == logged);     // conditionals log nothing
            // kernels do not run here: the words are what the host wrote; clearing them is one call
            EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words == pattern);
            EXPECT(qsv_ensemble_bits_write(st, n, nullptr) == QSV_OK && qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words[0] == 0 && words.back() == 0);
            EXPECT(qsv_destroy(st) == QSV_OK);     // with the log, the workspace and the bits allocated
        }

    // ---- the member size: fixed while the log is not empty; the bits are re-made and zeroed when it changes -------------------------
    {
        qsv_state *st = nullptr;
        const int n = 3, b = 3, members = 8, total = 300;
        EXPECT(qsv_create(n + b, 0, &st) == QSV_OK);
        std::vector<uint64_t> words(16, 7), ones(16, ~0ull);
        // no log yet: the bits may be read at one member size and then at another
        EXPECT(qsv_ensemble_bits_write(st, n, ones.data()) == QSV_OK);
        EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words[0] == ~0ull && words[7] == ~0ull && words[8] == 7);
        EXPECT(qsv_ensemble_bits_read(st, n - 1, words.data()) == QSV_OK && words[0] == 0 && words[15] == 0);      // re-made, zeroed
        EXPECT(qsv_ensemble_bits_write(st, n, ones.data()) == QSV_OK);
        std::vector<double> u(members, 0.25), u16(16, 0.25);
        // measurements and channels mixed, more than the device slots
        for (int i = 0; i < total; ++i) {
            const int q = i % n;
            if (i % 3 == 0) EXPECT(qsv_ensemble_measure(st, n, q, Y0, Y1, i % 2, i % 64, u.data(), nullptr) == QSV_OK);
            else EXPECT(qsv_ensemble_apply_channel(st, n, i % 3 == 1 ? mixed : one, &q, u.data(), nullptr) == QSV_OK);
            if (i % 50 == 0) EXPECT(qsv_ensemble_apply_conditional(st, n, 1, &q, H, 1, 2) == QSV_OK);
        }
        // 300 steps pending: another member size is refused by all four calls until they are read, before any launch
        const unsigned long before = qsv_stub_launches;
        const int q = 0;
        EXPECT(qsv_ensemble_measure(st, n - 1, q, Z0, Z1, 0, 0, u16.data(), nullptr) == QSV_ESTATE);
        EXPECT(qsv_ensemble_apply_conditional(st, n - 1, 1, &q, H, 0, 0) == QSV_ESTATE);
        EXPECT(qsv_ensemble_bits_read(st, n - 1, words.data()) == QSV_ESTATE && qsv_ensemble_bits_write(st, n - 1, nullptr) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words[0] == ~0ull);                     // the same size: fine, and untouched
        std::vector<int32_t> branches(static_cast<size_t>(total) * members + 1, -5);
        std::vector<double> probs(static_cast<size_t>(total) * members + 1, -5.0);
        uint64_t steps = 0;
        EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == total);
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total, &steps) == QSV_OK && steps == total);
        bool complete = branches.back() == -5 && probs.back() == -5.0;
        for (size_t e = 0; e + 1 < branches.size(); ++e) complete = complete && branches[e] == 0 && probs[e] == 0.0;   // the stand-in's zeroed memory
        EXPECT(complete);
        // now the member size may change: workspace and bits are re-made
        EXPECT(qsv_ensemble_measure(st, n - 1, q, Z0, Z1, 0, 5, u16.data(), nullptr) == QSV_OK);
        EXPECT(qsv_ensemble_bits_read(st, n - 1, words.data()) == QSV_OK && words[0] == 0 && words[15] == 0);
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total, &steps) == QSV_OK && steps == 1);
        // a channel call changes the member size back; the bits follow at their next use
        EXPECT(qsv_ensemble_apply_channel(st, n, one, &q, u.data(), nullptr) == QSV_OK);
        EXPECT(qsv_ensemble_bits_read(st, n - 1, words.data()) == QSV_ESTATE);
        EXPECT(qsv_ensemble_apply_conditional(st, n, 1, &q, H, 0, 0) == QSV_OK);
        EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && words[0] == 0 && words[7] == 0);
        EXPECT(qsv_destroy(st) == QSV_OK);                                 // with one entry left in the log
    }

    // ---- deferring registers: refusals leave the queue alone, a valid call flushes it first ------------------------------------------
    for (int n : {9, 13}) {
        const int b = 3;
        qsv_state *st = nullptr, *twin = nullptr;
        EXPECT(qsv_create(n + b, 0, &st) == QSV_OK && qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_create(n + b, 0, &twin) == QSV_OK && qsv_set_option(twin, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_apply_1q(st, b + 3, H) == QSV_OK && qsv_apply_1q(twin, b + 3, H) == QSV_OK);
        const Stats start = stats_of(st);
        EXPECT(start.queued == 1 && start.launched == 0);
        call_refusals(st, n, b, modes, view);
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_flush(twin) == QSV_OK);
        const unsigned long flush_cost = qsv_stub_launches - before;
        EXPECT(flush_cost >= 1);
        const std::vector<double> u(size_t(1) << b, 0.4);
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_measure(st, n, n - 1, Y0, Y1, 0, 3, u.data(), nullptr) == QSV_OK);
        EXPECT(stats_of(st).launched == stats_of(twin).launched && qsv_stub_launches - before == flush_cost + MEASURE_LAUNCHES);
        EXPECT(qsv_apply_1q(st, b + 1, H) == QSV_OK && qsv_apply_1q(twin, b + 1, H) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_flush(twin) == QSV_OK);
        const unsigned long second_flush = qsv_stub_launches - before;
        const int qs[2] = {n - 1, 2};
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_conditional(st, n, 2, qs, CX, 8, 0) == QSV_OK && qsv_stub_launches - before == second_flush + CONDITIONAL_LAUNCHES);
        EXPECT(stats_of(st).launched == stats_of(twin).launched);
        // the bits calls do not touch the amplitudes: the queue stays
        EXPECT(qsv_apply_1q(st, b, H) == QSV_OK);
        std::vector<uint64_t> words(u.size(), 7);
        const Stats pending = stats_of(st);
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_bits_read(st, n, words.data()) == QSV_OK && qsv_ensemble_bits_write(st, n, words.data()) == QSV_OK);
        EXPECT(stats_of(st).launched == pending.launched && qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK && qsv_destroy(twin) == QSV_OK);   // with a gate pending, a step in the log and the bits allocated
    }

    EXPECT(qsv_channel_destroy(one) == QSV_OK && qsv_channel_destroy(mixed) == QSV_OK);
    EXPECT(qsv_destroy(modes) == QSV_OK && qsv_destroy(view) == QSV_OK);
    std::free(view_memory);
    return finish("ensemble_control");
}

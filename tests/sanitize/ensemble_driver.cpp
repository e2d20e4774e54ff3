// TEST INFRASTRUCTURE: drives the host side of the trajectory-ensemble entry points (qsv_ensemble_broadcast,
// qsv_ensemble_apply_channel, qsv_ensemble_log_read, qsv_ensemble_norm2, qsv_ensemble_expect_pauli_sum) -- every refusal (a
// channel on another device and a view too), valid calls for members of 1 to 16 qubits x 1 to 64 members on every target
// bit, the launch counts and a log longer than its device slots -- under ASan + UBSan against hip_stub.cpp (device memory
// is zeroed host memory and kernels do not run, so every branch "chosen on the device" reads back as (0, 0.0)).
// Launches are counted: a general call adds the same three (read pass, select, update pass) whatever the number of Kraus
// operators and of members, a mixed-unitary call has no read pass.
// Walks: null pointers, a member size outside k .. n_total, target and term qubits outside a member or repeated, a draw
// outside [0, 1) or a forced branch out of range in any member, mode registers, views, a channel on another device -- each
// refused before any launch and with the deferred queue left as it was.  A log of 300 steps, more than its device slots, is
// read back complete; what it holds is the stand-in's zeroed memory, its order is checked on the device
// (tests/test_gpu_ensemble.py).
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "driver_common.h"

constexpr int GENERAL_LAUNCHES = 3;     // read pass, select, update pass
constexpr int MIXED_LAUNCHES = 2;       // select, update pass
constexpr int PASS_LAUNCHES = 2;        // a Pauli pass and the per-member sum of its parts

static qsv_channel *make(int k, int count, const std::vector<double> &kraus, int want_mixed) {
    qsv_channel *c = nullptr;
    int mixed = -1;
    EXPECT(qsv_channel_create(k, count, kraus.data(), 0, &c) == QSV_OK && c != nullptr);
    EXPECT(qsv_channel_info(c, nullptr, nullptr, &mixed) == QSV_OK && mixed == want_mixed);
    return c;
}

// every refusal on a register of n + b qubits read as 2^b members of n >= 2 qubits; nothing may be launched, logged or flushed
static void call_refusals(qsv_state *st, int n, int b, qsv_channel *one, qsv_channel *two, qsv_channel *mixed, qsv_state *modes, qsv_state *view) {
    const unsigned long before = qsv_stub_launches;
    const Stats was = stats_of(st);
    const size_t members = size_t(1) << b;
    const std::vector<double> u(members, 0.5);
    std::vector<double> bad_u = u;
    std::vector<int> forced(members, -1);
    const int q0[2] = {0, 1};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (qsv_channel *c : {one, mixed}) {
        EXPECT(qsv_ensemble_apply_channel(nullptr, n, c, q0, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, n, nullptr, q0, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, n, c, nullptr, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, n, c, q0, nullptr, nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, 0, c, q0, u.data(), nullptr) == QSV_EINVAL);            // below k
        EXPECT(qsv_ensemble_apply_channel(st, -1, c, q0, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, n + b + 1, c, q0, u.data(), nullptr) == QSV_EINVAL);    // above n_total
        for (double wrong : {1.0, -0.1, nan, 2.0}) {                                                  // in the last member only
            bad_u.back() = wrong;
            EXPECT(qsv_ensemble_apply_channel(st, n, c, q0, bad_u.data(), nullptr) == QSV_EINVAL);
            EXPECT(qsv_ensemble_apply_channel(st, n, c, q0, bad_u.data(), forced.data()) == QSV_EINVAL);
        }
        for (int wrong : {-2, 2, 99}) {                                                               // both have two operators
            forced.back() = wrong;
            EXPECT(qsv_ensemble_apply_channel(st, n, c, q0, u.data(), forced.data()) == QSV_EINVAL);
        }
        forced.back() = -1;
        const int low = -1, high = n, member_bit = n + b - 1;
        EXPECT(qsv_ensemble_apply_channel(st, n, c, &low, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(st, n, c, &high, u.data(), nullptr) == QSV_EINVAL);        // a qubit of the register, not of a member
        if (b > 0) EXPECT(qsv_ensemble_apply_channel(st, n, c, &member_bit, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_channel(modes, 1, c, q0, u.data(), nullptr) == QSV_ESTATE);
        EXPECT(qsv_ensemble_apply_channel(view, 2, c, q0, u.data(), nullptr) == QSV_EINVAL);
    }
    const int twice[2] = {0, 0}, outside[2] = {0, n};
    EXPECT(qsv_ensemble_apply_channel(st, n, two, twice, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_channel(st, n, two, outside, u.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_channel(st, 1, two, q0, u.data(), nullptr) == QSV_EINVAL);              // members smaller than the channel
    // the read-outs and the broadcast
    std::vector<double> out(members, 7.0), per_term(members * 2, 7.0);
    const int offsets[3] = {0, 1, 3}, qubits[3] = {0, 1, 0}, bad_qubits[3] = {0, 1, n}, repeated[3] = {0, 1, 1}, late[3] = {1, 2, 3}, back[3] = {0, 2, 1};
    const char letters[3] = {'Z', 'x', 'Y'}, bad_letters[3] = {'Z', 'Q', 'Y'};
    EXPECT(qsv_ensemble_norm2(nullptr, n, out.data()) == QSV_EINVAL && qsv_ensemble_norm2(st, n, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_norm2(st, 0, out.data()) == QSV_EINVAL && qsv_ensemble_norm2(st, n + b + 1, out.data()) == QSV_EINVAL);
    EXPECT(qsv_ensemble_norm2(modes, 1, out.data()) == QSV_ESTATE && qsv_ensemble_norm2(view, 2, out.data()) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(nullptr, n, 2, offsets, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, qubits, letters, nullptr, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, -1, offsets, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, nullptr, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, nullptr, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, qubits, nullptr, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, bad_qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, repeated, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, offsets, qubits, bad_letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 2, back, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(st, 1, 2, late, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);   // qubit 1 of 1-qubit members
    EXPECT(qsv_ensemble_expect_pauli_sum(st, 0, 2, offsets, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_expect_pauli_sum(modes, 1, 2, offsets, qubits, letters, nullptr, out.data(), nullptr) == QSV_ESTATE);
    EXPECT(qsv_ensemble_expect_pauli_sum(view, 2, 2, offsets, qubits, letters, nullptr, out.data(), nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_broadcast(nullptr, n) == QSV_EINVAL && qsv_ensemble_broadcast(st, -1) == QSV_EINVAL);
    EXPECT(qsv_ensemble_broadcast(st, n + b + 1) == QSV_EINVAL && qsv_ensemble_broadcast(modes, 1) == QSV_ESTATE && qsv_ensemble_broadcast(view, 1) == QSV_EINVAL);
    EXPECT(out[0] == 7.0 && out.back() == 7.0 && per_term[0] == 7.0);
    const Stats now = stats_of(st);
    EXPECT(now.queued == was.queued && now.launched == was.launched);
    EXPECT(qsv_stub_launches == before);
}

int main() {
    qsv_channel *one = make(1, 2, amplitude_damping(0.3), 0), *one16 = make(1, 16, general(1, 16), 0), *two = make(2, 3, general(2, 3), 0);
    qsv_channel *two16 = make(2, 16, general(2, 16), 0), *mixed = make(1, 2, bit_flip(0.25), 1);
    qsv_state *modes = nullptr, *view = nullptr;
    EXPECT(qsv_create_qudit(2, 3, 0, &modes) == QSV_OK);
    void *view_memory = std::calloc(16, 16);
    EXPECT(qsv_create_view(4, 0, view_memory, 16, nullptr, &view) == QSV_OK);

    // ---- members of 1 to 16 qubits x 1 to 64 members: refusals, then valid calls on every target bit ----------------------------
    for (int n = 1; n <= 16; ++n)
        for (int b = 0; b <= 6; ++b) {
            qsv_state *st = nullptr;
            const size_t members = size_t(1) << b;
            EXPECT(qsv_create(n + b, 0, &st) == QSV_OK);
            EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 0) == QSV_OK);
            if (n >= 2) call_refusals(st, n, b, one, two, mixed, modes, view);
            std::vector<double> u(members);
            std::vector<int> forced(members);
            for (size_t m = 0; m < members; ++m) {
                u[m] = (m + 0.5) / members;
                forced[m] = static_cast<int>(m % 3) - 1;
            }
            char name[96] = "", want[96];
            uint64_t logged = 0;
            for (int cap : {0, 2}) {
                EXPECT(qsv_set_option(st, QSV_OPT_GRID_CAP, cap) == QSV_OK);
                for (int variant : {0, 1}) {
                    if (variant == 1 && (cap != 0 || (b != 0 && b != 3))) continue;
                    EXPECT(qsv_set_option(st, QSV_OPT_READOUT_VARIANT, variant) == QSV_OK);
                    for (int q = 0; q < n; ++q) {
                        for (qsv_channel *c : {one, one16}) {
                            const unsigned long before = qsv_stub_launches;
                            EXPECT(qsv_ensemble_apply_channel(st, n, c, &q, u.data(), nullptr) == QSV_OK && qsv_stub_launches - before == GENERAL_LAUNCHES);
                            EXPECT(qsv_ensemble_apply_channel(st, n, c, &q, u.data(), forced.data()) == QSV_OK && qsv_stub_launches - before == 2 * GENERAL_LAUNCHES);
                            logged += 2;
                        }
                        // bit n-1-q is a lane bit where a member has at least 6 qubits and the streaming forms are on
                        const bool lane = n >= 6 && variant == 0 && n - 1 - q < 6;
                        std::snprintf(want, sizeof(want), "k_ens_channel_apply<1, %d, true> after k_ens_channel_rdm", lane ? 1 : 0);
                        EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        const unsigned long before = qsv_stub_launches;
                        EXPECT(qsv_ensemble_apply_channel(st, n, mixed, &q, u.data(), nullptr) == QSV_OK && qsv_stub_launches - before == MIXED_LAUNCHES);
                        std::snprintf(want, sizeof(want), "k_ens_channel_apply<1, %d, true> after k_ens_channel_select", lane ? 1 : 0);
                        EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        ++logged;
                    }
                    for (int q0 = 0; q0 < n; ++q0)
                        for (int q1 = 0; q1 < n; ++q1) {
                            if (q0 == q1 || (n > 8 && (q0 * 7 + q1 * 3 + n + b) % 5)) continue;     // a fifth of the pairs of the larger members
                            const int qs[2] = {q0, q1};
                            for (qsv_channel *c : {two, two16}) {
                                const unsigned long before = qsv_stub_launches;
                                EXPECT(qsv_ensemble_apply_channel(st, n, c, qs, u.data(), forced.data()) == QSV_OK && qsv_stub_launches - before == GENERAL_LAUNCHES);
                                ++logged;
                            }
                            const int lanes = n >= 6 && variant == 0 ? (n - 1 - q0 < 6) + (n - 1 - q1 < 6) : 0;
                            std::snprintf(want, sizeof(want), "k_ens_channel_apply<2, %d, true> after k_ens_channel_rdm", lanes);
                            EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        }
                }
            }
            uint64_t steps = 0;
            EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == logged);
            // read-outs: one launch pair per pass, numbers for every member
            std::vector<double> out(members, 7.0), per_term(members * 3, 7.0);
            unsigned long before = qsv_stub_launches;
            EXPECT(qsv_ensemble_norm2(st, n, out.data()) == QSV_OK && qsv_stub_launches - before == PASS_LAUNCHES && out[0] == 0.0 && out.back() == 0.0);
            const int offsets[4] = {0, 1, 2, 2}, qubits[2] = {0, n - 1};
            const char letters[2] = {'Z', 'X'};
            const double coeffs[3] = {1.0, -0.5, 0.25};
            before = qsv_stub_launches;
            out.assign(members, 7.0);
            EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 3, offsets, qubits, letters, coeffs, out.data(), per_term.data()) == QSV_OK);
            EXPECT(qsv_stub_launches - before == 2 * PASS_LAUNCHES && out[0] == 0.0 && out.back() == 0.0 && per_term.back() == 0.0);   // {Z, identity} and {X}
            before = qsv_stub_launches;
            EXPECT(qsv_ensemble_expect_pauli_sum(st, n, 0, nullptr, nullptr, nullptr, nullptr, out.data(), nullptr) == QSV_OK && qsv_stub_launches == before);
            EXPECT(qsv_ensemble_broadcast(st, n) == QSV_OK && qsv_ensemble_broadcast(st, n + b) == QSV_OK && qsv_ensemble_broadcast(st, 0) == QSV_OK);
            // qsv_destroy frees what is left of the log and the workspace (the leak check of this program says so)
            EXPECT(qsv_destroy(st) == QSV_OK);
        }

    // ---- the log: longer than the device slots, complete; the member size is fixed while it is not empty ---------------------------
    {
        qsv_state *st = nullptr;
        const int n = 3, b = 3, members = 8, total = 300;
        EXPECT(qsv_create(n + b, 0, &st) == QSV_OK);
        uint64_t steps = 99;
        int32_t none = 7;
        double nothing = 7.0;
        EXPECT(qsv_ensemble_log_read(nullptr, &none, &nothing, 1, &steps) == QSV_EINVAL);
        EXPECT(qsv_ensemble_log_read(st, &none, &nothing, 1, nullptr) == QSV_EINVAL);
        EXPECT(qsv_ensemble_log_read(st, nullptr, &nothing, 1, &steps) == QSV_EINVAL && qsv_ensemble_log_read(st, &none, nullptr, 1, &steps) == QSV_EINVAL);
        EXPECT(qsv_ensemble_log_read(st, &none, &nothing, 1, &steps) == QSV_OK && steps == 0 && none == 7);     // nothing logged yet
        std::vector<double> u(members, 0.25);
        for (int i = 0; i < total; ++i) {
            const int q = i % n;
            EXPECT(qsv_ensemble_apply_channel(st, n, i % 3 == 1 ? mixed : one16, &q, u.data(), nullptr) == QSV_OK);
        }
        // 300 steps pending: another member size is refused until they are read, before any launch
        const unsigned long before = qsv_stub_launches;
        const int q = 0;
        std::vector<double> u16(16, 0.25);
        EXPECT(qsv_ensemble_apply_channel(st, n - 1, one, &q, u16.data(), nullptr) == QSV_ESTATE && qsv_stub_launches == before);
        std::vector<int32_t> branches(static_cast<size_t>(total) * members + 1, -5);
        std::vector<double> probs(static_cast<size_t>(total) * members + 1, -5.0);
        EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == total);
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total - 1, &steps) == QSV_OK && steps == total && branches[0] == -5);
        EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == total);              // nothing was cleared
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total, &steps) == QSV_OK && steps == total);
        bool complete = branches.back() == -5 && probs.back() == -5.0;
        for (size_t e = 0; e + 1 < branches.size(); ++e) complete = complete && branches[e] == 0 && probs[e] == 0.0;   // the stand-in's zeroed memory
        EXPECT(complete);
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total, &steps) == QSV_OK && steps == 0);   // read and cleared
        // now the member size may change: the workspace is re-made
        EXPECT(qsv_ensemble_apply_channel(st, n - 1, one, &q, u16.data(), nullptr) == QSV_OK);
        EXPECT(qsv_ensemble_log_read(st, branches.data(), probs.data(), total, &steps) == QSV_OK && steps == 1 && branches[15] == 0 && branches[16] == 0);
        // the single-register log is another log
        uint64_t count = 99;
        EXPECT(qsv_apply_channel(st, one, &q, 0.5, -1) == QSV_OK && qsv_ensemble_apply_channel(st, n, one, &q, u.data(), nullptr) == QSV_OK);
        EXPECT(qsv_channel_log_read(st, nullptr, nullptr, 0, &count) == QSV_OK && count == 1);
        EXPECT(qsv_ensemble_log_read(st, nullptr, nullptr, 0, &steps) == QSV_OK && steps == 1);
        EXPECT(qsv_destroy(st) == QSV_OK);                                 // with one entry left in each log
    }

    // ---- deferring registers: refusals leave the queue alone, a valid call flushes it first ------------------------------------------
    for (int n : {9, 13}) {
        const int b = 3;
        qsv_state *st = nullptr, *twin = nullptr;
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_create(n + b, 0, &st) == QSV_OK && qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_create(n + b, 0, &twin) == QSV_OK && qsv_set_option(twin, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_apply_1q(st, b + 3, h) == QSV_OK && qsv_apply_1q(twin, b + 3, h) == QSV_OK);
        const Stats start = stats_of(st);
        EXPECT(start.queued == 1 && start.launched == 0);
        call_refusals(st, n, b, one, two, mixed, modes, view);
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_flush(twin) == QSV_OK);
        const unsigned long flush_cost = qsv_stub_launches - before;
        EXPECT(flush_cost >= 1);
        const std::vector<double> u(size_t(1) << b, 0.4);
        const int qs[2] = {n - 1, 2};
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_channel(st, n, two16, qs, u.data(), nullptr) == QSV_OK);
        EXPECT(stats_of(st).launched == stats_of(twin).launched && qsv_stub_launches - before == flush_cost + GENERAL_LAUNCHES);
        // a mixed-unitary call flushes too: its matrix differs from member to member
        EXPECT(qsv_apply_1q(st, b + 1, h) == QSV_OK && qsv_apply_1q(twin, b + 1, h) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_flush(twin) == QSV_OK);
        const unsigned long second_flush = qsv_stub_launches - before;
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_channel(st, n, mixed, qs, u.data(), nullptr) == QSV_OK && qsv_stub_launches - before == second_flush + MIXED_LAUNCHES);
        // the read-outs flush as well
        EXPECT(qsv_apply_1q(st, b, h) == QSV_OK);
        const Stats pending = stats_of(st);
        std::vector<double> out(u.size());
        EXPECT(qsv_ensemble_norm2(st, n, out.data()) == QSV_OK && stats_of(st).launched > pending.launched);
        EXPECT(qsv_apply_1q(st, b, h) == QSV_OK);
        EXPECT(qsv_destroy(st) == QSV_OK && qsv_destroy(twin) == QSV_OK);   // with a gate pending and two steps in the log
    }

    // ---- a channel on another device ---------------------------------------------------------------------------------------------------
    {
        qsv_stub_devices = 2;
        qsv_state *far = nullptr, *near = nullptr;
        qsv_channel *far_channel = nullptr;
        EXPECT(qsv_create(8, 1, &far) == QSV_OK && qsv_create(8, 0, &near) == QSV_OK);
        EXPECT(qsv_channel_create(1, 2, amplitude_damping(0.3).data(), 1, &far_channel) == QSV_OK);
        const unsigned long before = qsv_stub_launches;
        const int q = 2;
        const std::vector<double> u(4, 0.5);
        uint64_t steps = 99;
        for (qsv_channel *c : {one, mixed}) EXPECT(qsv_ensemble_apply_channel(far, 6, c, &q, u.data(), nullptr) == QSV_EINVAL);      // made on device 0
        EXPECT(qsv_ensemble_apply_channel(near, 6, far_channel, &q, u.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_ensemble_log_read(far, nullptr, nullptr, 0, &steps) == QSV_OK && steps == 0);
        EXPECT(qsv_ensemble_apply_channel(far, 6, far_channel, &q, u.data(), nullptr) == QSV_OK && qsv_ensemble_apply_channel(near, 6, one, &q, u.data(), nullptr) == QSV_OK);
        EXPECT(qsv_destroy(far) == QSV_OK && qsv_destroy(near) == QSV_OK && qsv_channel_destroy(far_channel) == QSV_OK);
        qsv_stub_devices = 1;
    }

    for (qsv_channel *c : {one, one16, two, two16, mixed}) EXPECT(qsv_channel_destroy(c) == QSV_OK);
    EXPECT(qsv_destroy(modes) == QSV_OK && qsv_destroy(view) == QSV_OK);
    std::free(view_memory);
    return finish("ensemble");
}

// TEST INFRASTRUCTURE: drives the host side of the noise entry points (qsv_channel_*, qsv_apply_channel,
// qsv_channel_log_read, qsv_density_expect_paulis) -- every refusal (a channel on another device too: qsv_stub_devices), the
// host-side branch pick of mixed-unitary channels, the launch shapes of the kernel path for 1 to 18 qubits and the branch
// log -- under ASan + UBSan against hip_stub.cpp
// (device memory is zeroed host memory and kernels do not run, so a branch "chosen on the device" reads back as (0, 0.0)).
// Launches are counted: a mixed-unitary call on a deferring register adds none at call time, a general call adds the same
// fixed number whatever the number of Kraus operators.
// Walks: null pointers, bad sizes and devices, draws outside [0, 1), forced branches out of range, qubits repeated or out of
// range, mode registers, a channel on another device, density registers with an odd number of qubits, bad term lists -- each
// refused before any launch and with the deferred queue left as it was -- and then valid calls for 1 to 18 qubits on every
// target bit, with and without the streaming forms and the grid cap.  A log of 900 entries, 600 of them in device slots, is
// read back complete and in call order.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "driver_common.h"

constexpr int GENERAL_LAUNCHES = 4;     // read pass, sum of the partials, select, update pass

// 16 two-qubit Paulis, equal weights: mixed-unitary (only X and Z letters, so every entry is real)
static std::vector<double> flat_two_qubit(int count) {
    std::vector<double> out(static_cast<size_t>(2) * 16 * count, 0.0);
    for (int j = 0; j < count; ++j)
        for (int r = 0; r < 4; ++r) {
            const int c = r ^ (j & 3);                                       // X letters
            const int sign = __builtin_popcount(r & (j >> 2)) & 1 ? -1 : 1;  // Z letters
            out[2 * (16 * static_cast<size_t>(j) + r * 4 + c)] = sign / std::sqrt(static_cast<double>(count));
        }
    return out;
}

static qsv_channel *make(int k, int count, const std::vector<double> &kraus, int want_mixed) {
    qsv_channel *c = nullptr;
    int kk = -1, nn = -1, mixed = -1;
    EXPECT(qsv_channel_create(k, count, kraus.data(), 0, &c) == QSV_OK && c != nullptr);
    EXPECT(qsv_channel_info(c, &kk, &nn, &mixed) == QSV_OK && kk == k && nn == count && mixed == want_mixed);
    EXPECT(qsv_channel_info(c, nullptr, nullptr, nullptr) == QSV_OK);
    return c;
}

// every refusal of qsv_apply_channel on a register of n qubits; nothing may be launched and the queue stays as it was
static void call_refusals(qsv_state *st, int n, qsv_channel *one, qsv_channel *two, qsv_channel *mixed, qsv_state *modes) {
    const unsigned long before = qsv_stub_launches;
    const Stats was = stats_of(st);
    const int q0[2] = {0, n > 1 ? 1 : 0};
    for (qsv_channel *c : {one, mixed}) {
        EXPECT(qsv_apply_channel(nullptr, c, q0, 0.5, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, nullptr, q0, 0.5, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, nullptr, 0.5, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, q0, 1.0, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, q0, -0.1, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, q0, std::numeric_limits<double>::quiet_NaN(), -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, q0, 1.0, 0) == QSV_EINVAL);             // also with a forced branch
        EXPECT(qsv_apply_channel(st, c, q0, 0.5, -2) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, q0, 0.5, 2) == QSV_EINVAL);             // both have two operators
        const int low = -1, high = n;
        EXPECT(qsv_apply_channel(st, c, &low, 0.5, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(st, c, &high, 0.5, -1) == QSV_EINVAL);
        EXPECT(qsv_apply_channel(modes, c, q0, 0.5, -1) == QSV_ESTATE);
    }
    const int twice[2] = {0, 0}, outside[2] = {0, n};
    EXPECT(qsv_apply_channel(st, two, twice, 0.5, -1) == QSV_EINVAL);
    EXPECT(qsv_apply_channel(st, two, outside, 0.5, -1) == QSV_EINVAL);
    const Stats now = stats_of(st);
    EXPECT(now.queued == was.queued && now.launched == was.launched);
    EXPECT(qsv_stub_launches == before);
}

static void density_calls(int n_rho) {
    qsv_state *rho = nullptr, *odd = nullptr, *modes = nullptr;
    EXPECT(qsv_create(2 * n_rho, 0, &rho) == QSV_OK && qsv_create(2 * n_rho + 1, 0, &odd) == QSV_OK && qsv_create_qudit(2, 3, 0, &modes) == QSV_OK);
    const int offsets[5] = {0, 0, 1, 3, 4}, qubits[4] = {0, n_rho - 1, 0, n_rho - 1};
    const char letters[4] = {'Z', 'x', 'Y', 'i'};
    double values[8] = {7, 7, 7, 7, 7, 7, 7, 7};
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_density_expect_paulis(nullptr, 4, offsets, qubits, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(odd, 4, offsets, qubits, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(modes, 4, offsets, qubits, letters, values) == QSV_ESTATE);
    EXPECT(qsv_density_expect_paulis(rho, -1, offsets, qubits, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 4, nullptr, qubits, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 4, offsets, qubits, letters, nullptr) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 4, offsets, nullptr, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 4, offsets, qubits, nullptr, values) == QSV_EINVAL);
    const int late[2] = {1, 2}, back[3] = {0, 2, 1};
    EXPECT(qsv_density_expect_paulis(rho, 1, late, qubits, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 2, back, qubits, letters, values) == QSV_EINVAL);
    const int one[2] = {0, 1}, pair[2] = {0, 2};
    const int outside = n_rho, negative = -1, repeated[2] = {0, 0};       // qubit n_rho is a column qubit of the register: refused
    const char bad = 'Q', zz[2] = {'Z', 'Z'};
    EXPECT(qsv_density_expect_paulis(rho, 1, one, &outside, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 1, one, &negative, letters, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 1, one, qubits, &bad, values) == QSV_EINVAL);
    EXPECT(qsv_density_expect_paulis(rho, 1, pair, repeated, zz, values) == QSV_EINVAL);
    std::vector<int> q65(65, 0);
    std::vector<char> l65(65, 'I');
    const int many[2] = {0, 65};
    EXPECT(qsv_density_expect_paulis(rho, 1, many, q65.data(), l65.data(), values) == QSV_EINVAL);
    EXPECT(qsv_stub_launches == before && values[0] == 7.0);
    EXPECT(qsv_density_expect_paulis(rho, 0, nullptr, nullptr, nullptr, nullptr) == QSV_OK && qsv_stub_launches == before);
    EXPECT(qsv_density_expect_paulis(rho, 4, offsets, qubits, letters, values) == QSV_OK && qsv_stub_launches == before + 1);
    EXPECT(values[0] == 0.0 && values[7] == 0.0);                          // eight numbers written
    char name[64] = "";
    EXPECT(qsv_last_kernel(rho, name, sizeof(name)) == QSV_OK && std::strcmp(name, "k_density_expect_paulis") == 0);
    for (qsv_state *st : {rho, odd, modes}) EXPECT(qsv_destroy(st) == QSV_OK);
}

int main() {
    const std::vector<double> ad = amplitude_damping(0.3), bf = bit_flip(0.25);
    {
        qsv_channel *c = nullptr;
        std::vector<double> nan = ad;
        nan[3] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(qsv_channel_create(1, 2, ad.data(), 0, nullptr) == QSV_EINVAL);
        EXPECT(qsv_channel_create(1, 2, nullptr, 0, &c) == QSV_EINVAL && c == nullptr);
        EXPECT(qsv_channel_create(0, 2, ad.data(), 0, &c) == QSV_EINVAL && qsv_channel_create(3, 2, ad.data(), 0, &c) == QSV_EINVAL && c == nullptr);
        EXPECT(qsv_channel_create(1, 0, ad.data(), 0, &c) == QSV_EINVAL && qsv_channel_create(1, 17, ad.data(), 0, &c) == QSV_EINVAL && c == nullptr);
        EXPECT(qsv_channel_create(1, 2, ad.data(), 1, &c) == QSV_EINVAL && qsv_channel_create(1, 2, ad.data(), -1, &c) == QSV_EINVAL && c == nullptr);
        EXPECT(qsv_channel_create(1, 2, nan.data(), 0, &c) == QSV_EINVAL && c == nullptr);
        EXPECT(qsv_channel_destroy(nullptr) == QSV_OK);
        EXPECT(qsv_channel_info(nullptr, nullptr, nullptr, nullptr) == QSV_EINVAL);
    }
    qsv_channel *one = make(1, 2, ad, 0), *one16 = make(1, 16, general(1, 16), 0), *two = make(2, 3, general(2, 3), 0);
    qsv_channel *two16 = make(2, 16, general(2, 16), 0), *mixed = make(1, 2, bf, 1), *mixed16 = make(2, 16, flat_two_qubit(16), 1);
    qsv_channel *single = make(1, 1, std::vector<double>{2, 0, 0, 0, 0, 0, 2, 0}, 1);   // 2 I: not trace preserving, still mixed-unitary
    qsv_state *modes = nullptr;
    EXPECT(qsv_create_qudit(2, 3, 0, &modes) == QSV_OK);
    std::vector<double> pauli5(32);                                        // operator 5 of flat_two_qubit, as a unitary
    for (int e = 0; e < 32; ++e) pauli5[e] = 4.0 * flat_two_qubit(16)[32 * 5 + e];

    // ---- 1 to 18 qubits: refusals, then valid calls on every kind of bit placement ---------------------------------------------
    for (int n = 1; n <= 18; ++n) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 0) == QSV_OK);
        call_refusals(st, n, one, two, mixed, modes);
        char name[96] = "";
        uint64_t logged = 0;
        for (int cap : {0, 2}) {
            EXPECT(qsv_set_option(st, QSV_OPT_GRID_CAP, cap) == QSV_OK);
            for (int variant : {0, 1}) {
                EXPECT(qsv_set_option(st, QSV_OPT_READOUT_VARIANT, variant) == QSV_OK);
                for (int q = 0; q < n; ++q) {
                    for (qsv_channel *c : {one, one16}) {
                        const unsigned long before = qsv_stub_launches;
                        EXPECT(qsv_apply_channel(st, c, &q, 0.3, -1) == QSV_OK && qsv_stub_launches - before == GENERAL_LAUNCHES);
                        EXPECT(qsv_apply_channel(st, c, &q, 0.0, c == one ? 1 : 15) == QSV_OK && qsv_stub_launches - before == 2 * GENERAL_LAUNCHES);
                        logged += 2;
                    }
                    // bit n-1-q is a lane bit only on a streaming register
                    const bool lane = n >= 14 && variant == 0 && n - 1 - q < 6;
                    char want[96];
                    std::snprintf(want, sizeof(want), "k_channel_apply<1, %d, true>", lane ? 1 : 0);
                    EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                    // the X branch, at once: what X costs through qsv_apply_1q
                    const double x[8] = {0, 0, 1, 0, 1, 0, 0, 0};
                    unsigned long before = qsv_stub_launches;
                    EXPECT(qsv_apply_1q(st, q, x) == QSV_OK);
                    const unsigned long direct = qsv_stub_launches - before;
                    before = qsv_stub_launches;
                    EXPECT(qsv_apply_channel(st, mixed, &q, 0.9, -1) == QSV_OK && qsv_stub_launches - before == direct && direct >= 1);
                    ++logged;
                }
                for (int q0 = 0; q0 < n; ++q0)
                    for (int q1 = 0; q1 < n; ++q1) {
                        if (q0 == q1 || (n > 8 && (q0 * 7 + q1 * 3 + n) % 5)) continue;     // a fifth of the pairs of the larger registers
                        const int qs[2] = {q0, q1};
                        for (qsv_channel *c : {two, two16}) {
                            const unsigned long before = qsv_stub_launches;
                            EXPECT(qsv_apply_channel(st, c, qs, 0.99, -1) == QSV_OK && qsv_stub_launches - before == GENERAL_LAUNCHES);
                            ++logged;
                        }
                        const int lanes = n >= 14 && variant == 0 ? (n - 1 - q0 < 6) + (n - 1 - q1 < 6) : 0;
                        char want[96];
                        std::snprintf(want, sizeof(want), "k_channel_apply<2, %d, true>", lanes);
                        EXPECT(qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0);
                        // a mixed-unitary branch costs what the same matrix costs through qsv_apply_2q
                        unsigned long before = qsv_stub_launches;
                        EXPECT(qsv_apply_2q(st, q0, q1, pauli5.data()) == QSV_OK);
                        const unsigned long direct = qsv_stub_launches - before;
                        before = qsv_stub_launches;
                        EXPECT(qsv_apply_channel(st, mixed16, qs, 0.5, 5) == QSV_OK && qsv_stub_launches - before == direct && direct >= 1);
                        ++logged;
                    }
            }
        }
        uint64_t count = 0;
        EXPECT(qsv_channel_log_read(st, nullptr, nullptr, 0, &count) == QSV_OK && count == logged);
        // qsv_destroy frees what is left of the log (the leak check of this program says so)
        EXPECT(qsv_destroy(st) == QSV_OK);
    }

    // ---- the log: longer than the device slots, complete and in call order ----------------------------------------------------------
    {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(3, 0, &st) == QSV_OK);
        uint64_t count = 99;
        int32_t none = 7;
        double nothing = 7.0;
        EXPECT(qsv_channel_log_read(nullptr, &none, &nothing, 1, &count) == QSV_EINVAL);
        EXPECT(qsv_channel_log_read(st, &none, &nothing, 1, nullptr) == QSV_EINVAL);
        EXPECT(qsv_channel_log_read(st, nullptr, &nothing, 1, &count) == QSV_EINVAL && qsv_channel_log_read(st, &none, nullptr, 1, &count) == QSV_EINVAL);
        EXPECT(qsv_channel_log_read(st, &none, &nothing, 1, &count) == QSV_OK && count == 0 && none == 7);    // nothing logged yet
        const int total = 900;                                            // 600 of them chosen "on the device": more than two drains
        for (int i = 0; i < total; ++i) {
            const int q = i % 3;
            if (i % 3 == 1) EXPECT(qsv_apply_channel(st, mixed, &q, 0.1, i % 2) == QSV_OK);    // forced 0 or 1, known to the host
            else EXPECT(qsv_apply_channel(st, one16, &q, 0.5, -1) == QSV_OK);
        }
        std::vector<int32_t> branches(total + 1, -5);
        std::vector<double> probs(total + 1, -5.0);
        EXPECT(qsv_channel_log_read(st, nullptr, nullptr, 0, &count) == QSV_OK && count == total);
        EXPECT(qsv_channel_log_read(st, branches.data(), probs.data(), total - 1, &count) == QSV_OK && count == total && branches[0] == -5);
        EXPECT(qsv_channel_log_read(st, nullptr, nullptr, 0, &count) == QSV_OK && count == total);            // nothing was cleared
        EXPECT(qsv_channel_log_read(st, branches.data(), probs.data(), total, &count) == QSV_OK && count == total);
        bool in_order = branches[total] == -5 && probs[total] == -5.0;
        for (int i = 0; i < total; ++i) {
            if (i % 3 == 1) in_order = in_order && branches[i] == i % 2 && std::fabs(probs[i] - (i % 2 ? 0.25 : 0.75)) < 1e-15;
            else in_order = in_order && branches[i] == 0 && probs[i] == 0.0;      // what the stand-in's zeroed device memory holds
        }
        EXPECT(in_order);
        EXPECT(qsv_channel_log_read(st, branches.data(), probs.data(), total, &count) == QSV_OK && count == 0);   // read and cleared
        // relative weights: 2 I is its own only branch with probability 1
        const int q = 0;
        EXPECT(qsv_apply_channel(st, single, &q, 0.7, -1) == QSV_OK);
        EXPECT(qsv_channel_log_read(st, branches.data(), probs.data(), 1, &count) == QSV_OK && count == 1 && branches[0] == 0 && probs[0] == 1.0);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }

    // ---- deferring registers ----------------------------------------------------------------------------------------------------------
    for (int n : {13, 16}) {
        qsv_state *st = nullptr, *twin = nullptr;
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_create(n, 0, &st) == QSV_OK && qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_create(n, 0, &twin) == QSV_OK && qsv_set_option(twin, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_apply_1q(st, 3, h) == QSV_OK && qsv_apply_1q(twin, 3, h) == QSV_OK);
        const Stats start = stats_of(st);
        EXPECT(start.queued == 1);
        call_refusals(st, n, one, two, mixed, modes);                     // the queue is left as it was
        // a mixed-unitary call adds no launch at call time: its gate waits in the queue with the others
        const unsigned long before = qsv_stub_launches;
        const int q = 5, qs[2] = {n - 1, 2};
        EXPECT(qsv_apply_channel(st, mixed, &q, 0.9, -1) == QSV_OK && qsv_apply_channel(twin, mixed, &q, 0.9, -1) == QSV_OK);
        EXPECT(qsv_apply_channel(st, mixed16, qs, 0.0, 9) == QSV_OK && qsv_apply_channel(twin, mixed16, qs, 0.0, 9) == QSV_OK);
        Stats now = stats_of(st);
        EXPECT(now.queued == start.queued + 2 && now.launched == start.launched && qsv_stub_launches == before);
        uint64_t count = 0;
        EXPECT(qsv_channel_log_read(st, nullptr, nullptr, 0, &count) == QSV_OK && count == 2);
        now = stats_of(st);
        EXPECT(now.launched == start.launched && qsv_stub_launches == before);     // counting the log flushes nothing
        // a general call flushes the queue -- at the cost qsv_flush has on a twin with the same queue -- then makes its own
        // fixed number of launches
        EXPECT(qsv_flush(twin) == QSV_OK);
        const unsigned long flush_cost = qsv_stub_launches - before;
        EXPECT(flush_cost >= 1);
        const unsigned long mark = qsv_stub_launches;
        EXPECT(qsv_apply_channel(st, two16, qs, 0.4, -1) == QSV_OK);
        now = stats_of(st);
        EXPECT(now.launched > start.launched && now.launched == stats_of(twin).launched);
        EXPECT(qsv_stub_launches - mark == flush_cost + GENERAL_LAUNCHES);
        int32_t branches[3];
        double probs[3];
        EXPECT(qsv_channel_log_read(st, branches, probs, 3, &count) == QSV_OK && count == 3);
        EXPECT(branches[0] == 1 && std::fabs(probs[0] - 0.25) < 1e-15 && branches[1] == 9 && std::fabs(probs[1] - 1.0 / 16) < 1e-15 && branches[2] == 0);
        // the Pauli traces of a deferring density register flush it
        EXPECT(qsv_apply_1q(st, 0, h) == QSV_OK);
        const Stats pending = stats_of(st);
        if (n % 2 == 0) {
            const int offsets[2] = {0, 1}, zq = 0;
            const char z = 'Z';
            double values[2];
            EXPECT(qsv_density_expect_paulis(st, 1, offsets, &zq, &z, values) == QSV_OK && stats_of(st).launched > pending.launched);
        }
        EXPECT(qsv_destroy(st) == QSV_OK);                                 // with a gate pending and the log empty
        EXPECT(qsv_destroy(twin) == QSV_OK);                               // with two entries left in its log
    }

    for (int n_rho : {2, 3, 6, 7}) density_calls(n_rho);

    // ---- a channel on another device ----------------------------------------------------------------------------------------------------
    {
        qsv_stub_devices = 2;
        qsv_state *far = nullptr, *near = nullptr;
        qsv_channel *far_channel = nullptr;
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_create(13, 1, &far) == QSV_OK && qsv_create(13, 0, &near) == QSV_OK);
        EXPECT(qsv_channel_create(1, 2, ad.data(), 1, &far_channel) == QSV_OK);
        EXPECT(qsv_set_option(far, QSV_OPT_DEFER, 2) == QSV_OK && qsv_apply_1q(far, 3, h) == QSV_OK);
        const Stats was = stats_of(far);
        const unsigned long before = qsv_stub_launches;
        const int q = 2;
        uint64_t count = 99;
        for (qsv_channel *c : {one, mixed}) EXPECT(qsv_apply_channel(far, c, &q, 0.5, -1) == QSV_EINVAL);      // made on device 0
        EXPECT(qsv_apply_channel(near, far_channel, &q, 0.5, -1) == QSV_EINVAL);
        EXPECT(stats_of(far).queued == was.queued && stats_of(far).launched == was.launched && qsv_stub_launches == before);
        EXPECT(qsv_channel_log_read(far, nullptr, nullptr, 0, &count) == QSV_OK && count == 0);
        EXPECT(qsv_apply_channel(far, far_channel, &q, 0.5, -1) == QSV_OK && qsv_apply_channel(near, one, &q, 0.5, -1) == QSV_OK);
        EXPECT(qsv_destroy(far) == QSV_OK && qsv_destroy(near) == QSV_OK && qsv_channel_destroy(far_channel) == QSV_OK);
        qsv_stub_devices = 1;
    }

    for (qsv_channel *c : {one, one16, two, two16, mixed, mixed16, single}) EXPECT(qsv_channel_destroy(c) == QSV_OK);
    EXPECT(qsv_destroy(modes) == QSV_OK);
    return finish("channel");
}

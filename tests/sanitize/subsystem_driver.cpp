// TEST INFRASTRUCTURE: drives the host side of the subsystem read-out (qsv_reduced_density_state,
// qsv_marginal_probabilities) -- every refusal (a density register on another device too: qsv_stub_devices), then valid calls
// for 1 to 18 qubits on several placements, with and without a grid cap and with a deferred queue pending -- under
// ASan + UBSan against hip_stub.cpp (device memory is zeroed host memory and kernels do not run, so a marginal reads back
// as zeros).  Launches are counted: the matrix-core form is two launches (k_subsys_tile, k_subsys_finish), the per-entry
// form one; the streaming marginal two (k_marginal_stream, k_sum_partials), the per-entry marginal one.
// Walks: null pointers, k = 0, k = 13, k > n, a marginal of 27 qubits, qubits repeated or out of range, a density register
// of the wrong size, on another device, equal to the ket or a view, mode registers -- each refused before any launch and
// with the deferred queue left as it was -- and then a call that finds gates queued on both registers.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <cstring>
#include <vector>

#include "driver_common.h"

static bool last_kernel_is(qsv_state *st, const char *want) {
    char name[96] = "";
    return qsv_last_kernel(st, name, sizeof(name)) == QSV_OK && std::strcmp(name, want) == 0;
}

// every refusal on a ket of n >= 2 qubits: nothing may be launched and the queue stays as it was
static void refusals(int n) {
    qsv_state *ket = nullptr, *rho = nullptr, *modes = nullptr, *small = nullptr, *view = nullptr, *owner = nullptr, *far = nullptr;
    EXPECT(qsv_create(n, 0, &ket) == QSV_OK && qsv_create(4, 0, &rho) == QSV_OK && qsv_create_qudit(2, 3, 0, &modes) == QSV_OK);
    EXPECT(qsv_create(2, 0, &small) == QSV_OK && qsv_create(4, 0, &owner) == QSV_OK);
    void *ptr = nullptr;
    EXPECT(qsv_device_ptr(owner, &ptr) == QSV_OK && ptr != nullptr);
    EXPECT(qsv_create_view(4, 0, ptr, 16, nullptr, &view) == QSV_OK);
    qsv_stub_devices = 2;
    EXPECT(qsv_create(4, 1, &far) == QSV_OK);
    if (n >= 22) {                                       // something pending, so that a refusal that flushed would show
        const double h[8] = {0.7071067811865476, 0, 0.7071067811865476, 0, 0.7071067811865476, 0, -0.7071067811865476, 0};
        EXPECT(qsv_apply_1q(ket, 0, h) == QSV_OK);
    }
    const unsigned long before = qsv_stub_launches;
    const Stats was = stats_of(ket);
    const int q2[2] = {0, 1};
    std::vector<double> out(4, 7.0);
    // null pointers
    EXPECT(qsv_reduced_density_state(nullptr, 2, q2, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 2, nullptr, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 2, q2, nullptr) == QSV_EINVAL);
    EXPECT(qsv_marginal_probabilities(nullptr, 2, q2, out.data()) == QSV_EINVAL);
    EXPECT(qsv_marginal_probabilities(ket, 2, nullptr, out.data()) == QSV_EINVAL);
    EXPECT(qsv_marginal_probabilities(ket, 2, q2, nullptr) == QSV_EINVAL);
    // k = 0, k = 13, k > n (the qubit lists are as long as the call may read)
    std::vector<int> many(28);
    for (int i = 0; i < 28; ++i) many[i] = i;
    EXPECT(qsv_reduced_density_state(ket, 0, q2, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, -1, q2, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 13, many.data(), rho) == QSV_EINVAL);           // k = 13, whatever n is
    EXPECT(qsv_reduced_density_state(small, 3, many.data(), rho) == QSV_EINVAL);          // k > n
    EXPECT(qsv_marginal_probabilities(ket, 0, q2, out.data()) == QSV_EINVAL);
    EXPECT(qsv_marginal_probabilities(small, 3, many.data(), out.data()) == QSV_EINVAL);
    EXPECT(qsv_marginal_probabilities(ket, 27, many.data(), out.data()) == QSV_EINVAL);  // marginal k = 27
    // qubits repeated or out of range
    const int twice[2] = {1, 1}, outside[2] = {0, n}, negative[2] = {-1, 0};
    for (const int *bad : {twice, outside, negative}) {
        EXPECT(qsv_reduced_density_state(ket, 2, bad, rho) == QSV_EINVAL);
        EXPECT(qsv_marginal_probabilities(ket, 2, bad, out.data()) == QSV_EINVAL);
    }
    // the density register: wrong size, another device, the ket itself, a view
    EXPECT(qsv_reduced_density_state(ket, 1, q2, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 2, q2, small) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 2, q2, far) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(rho, 2, q2, rho) == QSV_EINVAL);
    EXPECT(qsv_reduced_density_state(ket, 2, q2, view) == QSV_EINVAL);
    // mode registers
    EXPECT(qsv_reduced_density_state(modes, 1, q2, small) == QSV_ESTATE);
    EXPECT(qsv_reduced_density_state(ket, 2, q2, modes) == QSV_ESTATE);
    EXPECT(qsv_marginal_probabilities(modes, 1, q2, out.data()) == QSV_ESTATE);
    const Stats now = stats_of(ket);
    EXPECT(now.queued == was.queued && now.launched == was.launched);
    EXPECT(qsv_stub_launches == before && out[0] == 7.0 && out[3] == 7.0);
    for (qsv_state *st : {ket, rho, modes, small, view, owner, far}) EXPECT(qsv_destroy(st) == QSV_OK);
    qsv_stub_devices = 1;
}

// kept qubits of placement p (0 = the lowest bits, 1 = the top bits reversed, 2 = from bit 6 up, or rotated where they do not fit)
static std::vector<int> placement(int n, int k, int p) {
    std::vector<int> q(k);
    for (int j = 0; j < k; ++j) {
        if (p == 0) q[j] = n - 1 - j;
        else if (p == 1) q[j] = k - 1 - j;
        else if (n - 6 >= k) q[j] = n - 1 - (6 + j);
        else q[j] = (j + n / 2) % n;
    }
    return q;
}

static void valid_calls(int n, int cap) {
    qsv_state *ket = nullptr;
    EXPECT(qsv_create(n, 0, &ket) == QSV_OK);
    if (cap) EXPECT(qsv_set_option(ket, QSV_OPT_GRID_CAP, cap) == QSV_OK);
    for (int k = 1; k <= n && k <= 12; ++k) {
        if (n > 14 && k != 1 && k != 6 && k != 7 && k != 12 && k != n - 6) continue;
        qsv_state *rho = nullptr;
        EXPECT(qsv_create(2 * k, 0, &rho) == QSV_OK);
        for (int p = 0; p < 3; ++p) {
            const std::vector<int> q = placement(n, k, p);
            const bool tiled = n >= 14 && n - (k > 6 ? k : 6) >= 6;
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_reduced_density_state(ket, k, q.data(), rho) == QSV_OK);
            EXPECT(qsv_stub_launches == before + (tiled ? 2 : 1));
            EXPECT(last_kernel_is(ket, tiled ? "k_subsys_tile" : "k_subsys_entry"));
        }
        EXPECT(qsv_destroy(rho) == QSV_OK);
    }
    for (int k = 1; k <= n; ++k) {
        if (n > 14 && k > 3 && k != 12 && k != 13 && k != n) continue;
        for (int p = 0; p < 3; ++p) {
            const std::vector<int> q = placement(n, k, p);
            int high = 0;
            for (int j = 0; j < k; ++j) high += n - 1 - q[j] >= 6;
            const bool streaming = n >= 14 && k <= 12 && n - 6 - high >= 6;
            std::vector<double> out(static_cast<size_t>(1) << k, 7.0);     // exactly what the call may write
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_marginal_probabilities(ket, k, q.data(), out.data()) == QSV_OK);
            EXPECT(qsv_stub_launches == before + (streaming ? 2 : 1));
            EXPECT(last_kernel_is(ket, streaming ? "k_marginal_stream" : "k_marginal_entry"));
            EXPECT(out.front() == 0.0 && out.back() == 0.0);              // every entry written
        }
    }
    EXPECT(qsv_destroy(ket) == QSV_OK);
}

// a pending queue is applied before the read pass, on the ket and on the density register
static void flushes_both_queues() {
    const int n = 22, k = 11;                            // both registers have 22 qubits: both defer
    qsv_state *ket = nullptr, *rho = nullptr;
    EXPECT(qsv_create(n, 0, &ket) == QSV_OK && qsv_create(2 * k, 0, &rho) == QSV_OK);
    const double h[8] = {0.7071067811865476, 0, 0.7071067811865476, 0, 0.7071067811865476, 0, -0.7071067811865476, 0};
    EXPECT(qsv_apply_1q(ket, 3, h) == QSV_OK && qsv_apply_1q(rho, 5, h) == QSV_OK);
    EXPECT(stats_of(ket).queued == 1 && stats_of(ket).launched == 0 && stats_of(rho).queued == 1 && stats_of(rho).launched == 0);
    std::vector<int> q(k);
    for (int j = 0; j < k; ++j) q[j] = 2 * j;
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_reduced_density_state(ket, k, q.data(), rho) == QSV_OK);
    EXPECT(stats_of(ket).launched == 1 && stats_of(rho).launched == 1);
    EXPECT(qsv_stub_launches == before + 2 + 2);         // the two queued gates, then k_subsys_tile and k_subsys_finish
    EXPECT(qsv_apply_1q(ket, 4, h) == QSV_OK);
    std::vector<double> out(4, 7.0);
    const int two[2] = {21, 0};
    EXPECT(qsv_marginal_probabilities(ket, 2, two, out.data()) == QSV_OK && stats_of(ket).launched == 2);
    EXPECT(qsv_destroy(ket) == QSV_OK && qsv_destroy(rho) == QSV_OK);
}

int main() {
    for (int n : {2, 13, 16, 22}) refusals(n);
    for (int n = 1; n <= 18; ++n) valid_calls(n, 0);
    valid_calls(16, 2);
    flushes_both_queues();
    return finish("subsystem");
}

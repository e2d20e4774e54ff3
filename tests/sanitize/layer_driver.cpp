// TEST INFRASTRUCTURE: drives the host side of qsv_apply_layer and qsv_ensemble_apply_layer -- every validation branch, the
// planner, the staging of the per-member table and the launch of every pass -- under ASan + UBSan against hip_stub.cpp (device
// memory is zeroed host memory and kernels do not run).  The launches of every valid call are compared with the plan's passes
// (csrc/qsv_layer_plan.h, included here as the library includes it).
// Walks: null pointers, k out of range, repeated and out-of-range qubits, entries that are not finite, a mode register, a view
// and a bad member_qubits for the ensemble call -- each refused before any launch and with qsv_defer_stats unchanged, on plain
// and deferring registers -- then k = 0 and valid calls on plain registers of 1 to 20 qubits, ensembles, a deferring register
// and views.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <limits>
#include <numeric>
#include <vector>

#include "driver_common.h"
#include "qsv_layer_plan.h"

static uint64_t model_passes(int n, const std::vector<int> &qubits) {
    std::vector<int> bits;
    for (int q : qubits) bits.push_back(n - 1 - q);
    const uint64_t passes = qsv_layer_plan::layer_plan(n, bits).passes.size();
    EXPECT(passes == qsv_layer_plan::layer_passes(n, bits));
    return passes;
}

// `count` matrices, all different, none unitary
static std::vector<double> matrices(size_t count) {
    std::vector<double> m(count * 8);
    for (size_t i = 0; i < m.size(); ++i) m[i] = 0.25 + 0.001 * static_cast<double>(i % 977);
    return m;
}

static std::vector<int> all_qubits(int n) {
    std::vector<int> q(n);
    std::iota(q.begin(), q.end(), 0);
    return q;
}

static std::vector<std::vector<int>> lists(int n) {
    const std::vector<int> all = all_qubits(n);
    std::vector<int> scattered;
    for (int q = 0; q < n; ++q)
        if (q % 3 != 1) scattered.insert(q % 2 ? scattered.begin() : scattered.end(), q);
    return {all, std::vector<int>(all.rbegin(), all.rend()), {0}, {n - 1}, scattered};
}

static void expect_valid(qsv_state *st, int n, const std::vector<int> &qubits) {
    const int k = static_cast<int>(qubits.size());
    const std::vector<double> m = matrices(k);
    uint64_t passes = 99;
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_apply_layer(st, k, qubits.data(), m.data(), &passes) == QSV_OK);
    EXPECT(passes == model_passes(n, qubits) && qsv_stub_launches - before == passes);
    EXPECT(qsv_apply_layer(st, k, qubits.data(), m.data(), nullptr) == QSV_OK);
}

// member qubits of an ensemble of n-qubit members in a register of n_total qubits
static void expect_valid_ensemble(qsv_state *st, int n_total, int n, const std::vector<int> &qubits) {
    const int k = static_cast<int>(qubits.size());
    const std::vector<double> m = matrices((size_t{1} << (n_total - n)) * k);
    uint64_t passes = 99;
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_ensemble_apply_layer(st, n, k, qubits.data(), m.data(), &passes) == QSV_OK);
    EXPECT(passes == model_passes(n, qubits) && qsv_stub_launches - before == passes);
    EXPECT(qsv_ensemble_apply_layer(st, n, k, qubits.data(), m.data(), nullptr) == QSV_OK);
}

// every refusal of both calls on an owned register of n_total >= 3 qubits; nothing is launched or flushed
static void expect_refusals(qsv_state *st, int n_total) {
    const int n = n_total - 1;      // two members
    const std::vector<int> all = all_qubits(n_total);
    const std::vector<double> m = matrices(2 * static_cast<size_t>(n_total));
    std::vector<double> nan = m, inf = m;
    nan[5] = std::numeric_limits<double>::quiet_NaN();
    inf[8 * static_cast<size_t>(n) + 3] = std::numeric_limits<double>::infinity();      // in the second member's row
    const int out_of_range[1] = {n_total}, member_out_of_range[1] = {n}, negative[1] = {-1}, twice[2] = {1, 1};
    uint64_t passes = 99;
    const Stats stats = stats_of(st);
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_apply_layer(nullptr, 1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 1, nullptr, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 1, all.data(), nullptr, &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, -1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, n_total + 1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 1, out_of_range, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 1, negative, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 2, twice, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_apply_layer(st, 1, all.data(), nan.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(nullptr, n, 1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, 1, nullptr, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, 1, all.data(), nullptr, &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, -1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, n + 1, all.data(), m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, 1, member_out_of_range, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, 1, negative, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, 2, twice, m.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, n, all.data(), nan.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n, n, all.data(), inf.data(), &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, -1, 0, nullptr, nullptr, &passes) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_layer(st, n_total + 1, 1, all.data(), m.data(), &passes) == QSV_EINVAL);
    const Stats now = stats_of(st);
    EXPECT(now.queued == stats.queued && now.launched == stats.launched && qsv_stub_launches == before);
}

int main() {
    // ---- plain registers ---------------------------------------------------------------------------------------------------
    for (int n : {1, 2, 3, 5, 11, 12, 13, 14, 18, 19, 20}) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        // k = 0: nothing happens, no pointer needed
        EXPECT(qsv_apply_layer(st, 0, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_apply_layer(st, 0, nullptr, nullptr, nullptr) == QSV_OK);
        passes = 99;
        EXPECT(qsv_ensemble_apply_layer(st, n, 0, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_ensemble_apply_layer(st, 0, 0, nullptr, nullptr, nullptr) == QSV_OK);
        EXPECT(qsv_stub_launches == before);
        if (n >= 3) expect_refusals(st, n);
        for (const std::vector<int> &qubits : lists(n)) expect_valid(st, n, qubits);
        // ensembles: members of every size that gives at most 64 of them
        for (int member = std::max(1, n - 6); member <= n; ++member)
            for (const std::vector<int> &qubits : lists(member)) expect_valid_ensemble(st, n, member, qubits);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- a deferring register: a refused call leaves the queue alone, a valid one flushes it first ------------------------------
    {
        const int n = 14;
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_apply_1q(st, 3, h) == QSV_OK);
        const Stats queued = stats_of(st);
        EXPECT(queued.queued == 1 && queued.launched == 0);
        expect_refusals(st, n);
        const unsigned long before = qsv_stub_launches;
        const std::vector<int> all = all_qubits(n);
        const std::vector<double> m = matrices(n);
        uint64_t passes = 99;
        EXPECT(qsv_apply_layer(st, n, all.data(), m.data(), &passes) == QSV_OK);
        Stats now = stats_of(st);
        EXPECT(now.launched == queued.launched + 1 && now.queued == 1);     // the queued gate went out; the layer was never queued
        EXPECT(passes == 2 && passes == model_passes(n, all) && qsv_stub_launches == before + 1 + passes);
        EXPECT(qsv_apply_1q(st, 5, h) == QSV_OK);
        const std::vector<int> members = all_qubits(10);
        const std::vector<double> mm = matrices(16 * 10);
        const unsigned long mid = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_layer(st, 10, 10, members.data(), mm.data(), &passes) == QSV_OK);
        now = stats_of(st);
        EXPECT(now.launched == queued.launched + 2 && now.queued == 2 && passes == 1 && qsv_stub_launches == mid + 2);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- views: the single-register call works on them, the ensemble call refuses them ------------------------------------------
    for (int n : {6, 13}) {
        std::vector<double> mem(2ull << n, 0.0);
        qsv_state *st = nullptr;
        EXPECT(qsv_create_view(n, 0, mem.data(), 1ull << n, nullptr, &st) == QSV_OK);
        for (const std::vector<int> &qubits : lists(n)) expect_valid(st, n, qubits);
        const std::vector<int> all = all_qubits(n);
        const std::vector<double> m = matrices(2 * static_cast<size_t>(n));
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_layer(st, n - 1, n - 1, all.data(), m.data(), &passes) == QSV_EINVAL);
        EXPECT(qsv_ensemble_apply_layer(st, n, 0, nullptr, nullptr, &passes) == QSV_EINVAL);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- a mode register: refused by both ---------------------------------------------------------------------------------------
    {
        qsv_state *st = nullptr;
        EXPECT(qsv_create_qudit(3, 3, 0, &st) == QSV_OK);
        const int q[1] = {0};
        const std::vector<double> m = matrices(27);
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_layer(st, 1, q, m.data(), &passes) == QSV_ESTATE);
        EXPECT(qsv_apply_layer(st, 0, nullptr, nullptr, &passes) == QSV_ESTATE);
        EXPECT(qsv_ensemble_apply_layer(st, 1, 1, q, m.data(), &passes) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("layer");
}

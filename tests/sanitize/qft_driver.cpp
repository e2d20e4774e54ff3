// TEST INFRASTRUCTURE: drives the host side of qsv_apply_qft -- every validation branch, the planner and the launch of
// every pass and of the permutation -- under ASan + UBSan against hip_stub.cpp (device memory is zeroed host memory and
// kernels do not run).  The number of launches of every valid call is compared with the plan's (csrc/qsv_qft_plan.h,
// included here as the library includes it), plus one for the permutation.
// Walks: null pointers, a mode register, repeated and out-of-range qubits, unknown flag bits, a bad m -- each refused before
// any launch and with the deferred queue left alone -- then m = 0 and valid calls with every flag combination on plain
// registers of 1 to 20 qubits, on a deferring register and on a view.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <numeric>
#include <vector>

#include "driver_common.h"
#include "qsv_qft_plan.h"

// tile passes of the plan, plus one permutation where the reversal moves anything
static uint64_t model_launches(int n, const std::vector<int> &qubits, int flags) {
    std::vector<int> bits;
    for (int q : qubits) bits.push_back(n - 1 - q);
    const bool swaps = !(flags & QSV_QFT_NO_SWAPS) && qubits.size() >= 2;
    return qsv_qft_plan::qft_plan(n, bits, flags).size() + (swaps ? 1 : 0);
}

static void expect_valid(qsv_state *st, int n, const std::vector<int> &qubits) {
    for (int flags = 0; flags < 8; ++flags) {
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_qft(st, static_cast<int>(qubits.size()), qubits.data(), flags, &passes) == QSV_OK);
        EXPECT(passes == model_launches(n, qubits, flags) && qsv_stub_launches - before == passes);
        EXPECT(qsv_apply_qft(st, static_cast<int>(qubits.size()), qubits.data(), flags, nullptr) == QSV_OK);
    }
}

static std::vector<int> all_qubits(int n) {
    std::vector<int> q(n);
    std::iota(q.begin(), q.end(), 0);
    return q;
}

int main() {
    static_assert(QSV_QFT_INVERSE == qsv_qft_plan::INVERSE && QSV_QFT_NO_SWAPS == qsv_qft_plan::NO_SWAPS &&
                  QSV_QFT_CONJUGATE == qsv_qft_plan::CONJUGATE, "the header's flags are the planner's");
    for (int n : {1, 2, 5, 11, 12, 13, 14, 18, 20}) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        const std::vector<int> all = all_qubits(n);
        uint64_t passes = 99;
        // ---- m = 0: nothing happens, no pointer needed ----------------------------------------------------------------------
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_qft(st, 0, nullptr, 0, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_apply_qft(st, 0, all.data(), QSV_QFT_INVERSE, nullptr) == QSV_OK);
        // ---- refusals ------------------------------------------------------------------------------------------------------
        const int out_of_range[1] = {n}, negative[1] = {-1}, twice[2] = {0, 0};
        EXPECT(qsv_apply_qft(nullptr, 1, all.data(), 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 1, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, -1, all.data(), 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 65, all.data(), 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 1, out_of_range, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 1, negative, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 2, twice, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 1, all.data(), 8, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 1, all.data(), -1, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, 0, nullptr, 16, &passes) == QSV_EINVAL);
        EXPECT(qsv_stub_launches == before);
        // ---- valid calls: the whole register both ways round, single qubits, scattered subsets --------------------------------------
        expect_valid(st, n, all);
        expect_valid(st, n, std::vector<int>(all.rbegin(), all.rend()));
        expect_valid(st, n, {0});
        expect_valid(st, n, {n - 1});
        std::vector<int> scattered;
        for (int q = 0; q < n; ++q)
            if (q % 3 != 1) scattered.insert(q % 2 ? scattered.begin() : scattered.end(), q);
        expect_valid(st, n, scattered);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- a deferring register: a refused call leaves the queue alone, a valid one flushes it first ------------------------------
    {
        const int n = 13;
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_apply_1q(st, 3, h) == QSV_OK);
        const Stats queued = stats_of(st);
        const unsigned long before = qsv_stub_launches;
        const std::vector<int> all = all_qubits(n);
        const int bad[2] = {2, 13};
        uint64_t passes = 99;
        EXPECT(qsv_apply_qft(st, 2, bad, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_qft(st, n, all.data(), 32, &passes) == QSV_EINVAL);
        Stats now = stats_of(st);
        EXPECT(queued.queued == 1 && now.queued == 1 && now.launched == queued.launched && qsv_stub_launches == before);
        EXPECT(qsv_apply_qft(st, n, all.data(), 0, &passes) == QSV_OK);
        now = stats_of(st);
        EXPECT(now.launched == queued.launched + 1 && now.queued == 1);     // the queued gate went out; the transform was never queued
        EXPECT(passes == model_launches(n, all, 0) && passes == 3 && qsv_stub_launches == before + 1 + passes);
        expect_valid(st, n, {12, 0, 6, 5});
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- views on caller-owned memory (the permutation copies back into it), and a mode register (refused) -----------------------
    for (int n : {6, 13}) {
        std::vector<double> mem(2ull << n, 0.0);
        qsv_state *st = nullptr;
        EXPECT(qsv_create_view(n, 0, mem.data(), 1ull << n, nullptr, &st) == QSV_OK);
        expect_valid(st, n, all_qubits(n));
        expect_valid(st, n, {n - 1, 0, 2});
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    {
        qsv_state *st = nullptr;
        EXPECT(qsv_create_qudit(3, 3, 0, &st) == QSV_OK);
        const int q[1] = {0};
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_qft(st, 1, q, 0, &passes) == QSV_ESTATE);
        EXPECT(qsv_apply_qft(st, 0, nullptr, 0, &passes) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("Fourier-transform");
}

// TEST INFRASTRUCTURE: drives the host side of qsv_layer_adjoint and qsv_layer_transition -- every validation branch, the
// planner, the slices of the partial sums, the launch of every pass and the host's sums -- under ASan + UBSan against
// hip_stub.cpp (device memory is zeroed host memory and kernels do not run, so every value comes back 0).
// THE RULE: a valid call launches exactly the passes of qsv_apply_layer's plan (csrc/qsv_layer_plan.h, included here as the
// library includes it); the sums add no launch, the host adds the workgroups' partials after one copy.
// Walks: null handles, null arrays, k out of range, repeated and out-of-range qubits, entries that are not finite, registers of
// different sizes and devices, overlapping registers (the adjoint call only; bra == ket is accepted by the transition call), a
// mode register -- each refused before any launch and with qsv_defer_stats unchanged, on plain and deferring registers -- then
// k = 0 and valid calls for n = 1 .. 30 on all bits, bits 0..5, the top bit and random subsets.  Registers beyond 2^20 amplitudes
// are views of one address range reserved without access rights: nothing reads a register here.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <limits>
#include <numeric>
#include <random>
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

// all bits; index bits 0..5; the top bit; two random subsets in random order
static std::vector<std::vector<int>> lists(int n) {
    std::vector<std::vector<int>> out = {all_qubits(n), {}, {0}};
    for (int b = 0; b < std::min(n, 6); ++b) out[1].push_back(n - 1 - b);
    std::mt19937 rng(1000u + static_cast<unsigned>(n));
    for (int r = 0; r < 2; ++r) {
        std::vector<int> q = all_qubits(n);
        std::shuffle(q.begin(), q.end(), rng);
        q.resize(1 + rng() % static_cast<unsigned>(n));
        out.push_back(q);
    }
    return out;
}

static void expect_valid(qsv_state *psi, qsv_state *lambda, int n, const std::vector<int> &qubits) {
    const int k = static_cast<int>(qubits.size());
    const std::vector<double> m = matrices(k);
    std::vector<double> values(static_cast<size_t>(k) * 8, 7.0);
    uint64_t passes = 99;
    unsigned long before = qsv_stub_launches;
    EXPECT(qsv_layer_adjoint(psi, lambda, k, qubits.data(), m.data(), values.data(), &passes) == QSV_OK);
    EXPECT(passes == model_passes(n, qubits) && qsv_stub_launches - before == passes);
    for (double v : values) EXPECT(v == 0.0);          // every value was written: sums of the zeroed partials
    EXPECT(qsv_layer_adjoint(psi, lambda, k, qubits.data(), m.data(), values.data(), nullptr) == QSV_OK);
    for (qsv_state *bra : {lambda, psi}) {             // the transition call takes bra == ket
        std::fill(values.begin(), values.end(), 7.0);
        passes = 99;
        before = qsv_stub_launches;
        EXPECT(qsv_layer_transition(bra, psi, k, qubits.data(), values.data(), &passes) == QSV_OK);
        EXPECT(passes == model_passes(n, qubits) && qsv_stub_launches - before == passes);
        for (double v : values) EXPECT(v == 0.0);
    }
}

// every refusal of both calls on two registers of n >= 3 qubits; nothing is launched or flushed
static void expect_refusals(qsv_state *psi, qsv_state *lambda, qsv_state *smaller, qsv_state *modes, qsv_state *elsewhere, int n) {
    const std::vector<int> all = all_qubits(n);
    const std::vector<double> m = matrices(static_cast<size_t>(n));
    std::vector<double> nan = m, inf = m, values(static_cast<size_t>(n + 1) * 8, 7.0);
    nan[5] = std::numeric_limits<double>::quiet_NaN();
    inf[8 * static_cast<size_t>(n - 1) + 3] = std::numeric_limits<double>::infinity();
    const int out_of_range[1] = {n}, negative[1] = {-1}, twice[2] = {1, 1};
    uint64_t passes = 99;
    const Stats stats_psi = stats_of(psi), stats_lambda = stats_of(lambda);
    const unsigned long before = qsv_stub_launches;
    double *v = values.data();
    EXPECT(qsv_layer_adjoint(nullptr, lambda, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, nullptr, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, nullptr, m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, all.data(), nullptr, v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, all.data(), m.data(), nullptr, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, -1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, n + 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, out_of_range, m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, negative, m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 2, twice, m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, 1, all.data(), nan.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, lambda, n, all.data(), inf.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, smaller, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(smaller, psi, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, elsewhere, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_adjoint(psi, psi, 1, all.data(), m.data(), v, &passes) == QSV_EINVAL);          // the same handle
    EXPECT(qsv_layer_adjoint(psi, modes, 1, all.data(), m.data(), v, &passes) == QSV_ESTATE);
    EXPECT(qsv_layer_adjoint(modes, psi, 1, all.data(), m.data(), v, &passes) == QSV_ESTATE);
    EXPECT(qsv_layer_adjoint(modes, modes, 0, nullptr, nullptr, nullptr, &passes) == QSV_ESTATE);
    EXPECT(qsv_layer_transition(nullptr, psi, 1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, nullptr, 1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, 1, nullptr, v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, 1, all.data(), nullptr, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, -1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, n + 1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, 1, out_of_range, v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, 1, negative, v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(lambda, psi, 2, twice, v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(smaller, psi, 1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(elsewhere, psi, 1, all.data(), v, &passes) == QSV_EINVAL);
    EXPECT(qsv_layer_transition(modes, psi, 1, all.data(), v, &passes) == QSV_ESTATE);
    EXPECT(qsv_layer_transition(psi, modes, 1, all.data(), v, &passes) == QSV_ESTATE);
    for (double x : values) EXPECT(x == 7.0);          // a refused call writes no value
    const Stats now_psi = stats_of(psi), now_lambda = stats_of(lambda);
    EXPECT(now_psi.queued == stats_psi.queued && now_psi.launched == stats_psi.launched);
    EXPECT(now_lambda.queued == stats_lambda.queued && now_lambda.launched == stats_lambda.launched);
    EXPECT(qsv_stub_launches == before);
}

int main() {
    qsv_state *modes = nullptr;
    EXPECT(qsv_create_qudit(3, 3, 0, &modes) == QSV_OK);
    // one address range for the large views: reserved, never touched
    const int big = 30;
    const size_t reserve = (size_t{2} << big) * 16;
    void *range = mmap(nullptr, reserve, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    EXPECT(range != MAP_FAILED);
    if (range == MAP_FAILED) return finish("layer_adjoint");
    for (int n = 1; n <= big; ++n) {
        qsv_state *psi = nullptr, *lambda = nullptr;
        if (n <= 20) {
            EXPECT(qsv_create(n, 0, &psi) == QSV_OK);
            EXPECT(qsv_create(n, 0, &lambda) == QSV_OK);
        } else {
            char *base = static_cast<char *>(range);
            EXPECT(qsv_create_view(n, 0, base, 1ull << n, nullptr, &psi) == QSV_OK);
            EXPECT(qsv_create_view(n, 0, base + (size_t{16} << n), 1ull << n, nullptr, &lambda) == QSV_OK);
        }
        std::vector<double> values(8, 7.0);
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        // k = 0: nothing happens, no pointer needed, values untouched
        EXPECT(qsv_layer_adjoint(psi, lambda, 0, nullptr, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_layer_adjoint(psi, lambda, 0, nullptr, nullptr, values.data(), nullptr) == QSV_OK);
        passes = 99;
        EXPECT(qsv_layer_transition(lambda, psi, 0, nullptr, values.data(), &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_layer_transition(psi, psi, 0, nullptr, nullptr, nullptr) == QSV_OK);
        EXPECT(qsv_stub_launches == before && values[0] == 7.0 && values[7] == 7.0);
        if (n == 3 || n == 13) {
            qsv_state *smaller = nullptr, *elsewhere = nullptr;
            EXPECT(qsv_create(n - 1, 0, &smaller) == QSV_OK);
            qsv_stub_devices = 2;
            EXPECT(qsv_create(n, 1, &elsewhere) == QSV_OK);
            expect_refusals(psi, lambda, smaller, modes, elsewhere, n);
            // overlapping memory: a view into psi's second half against psi
            std::vector<double> mem(size_t{3} << n, 0.0);      // 1.5 registers
            qsv_state *first = nullptr, *second = nullptr;
            EXPECT(qsv_create_view(n, 0, mem.data(), 1ull << n, nullptr, &first) == QSV_OK);
            EXPECT(qsv_create_view(n, 0, mem.data() + (size_t{1} << n), 1ull << n, nullptr, &second) == QSV_OK);
            const std::vector<int> all = all_qubits(n);
            const std::vector<double> m = matrices(n);
            std::vector<double> v(static_cast<size_t>(n) * 8, 7.0);
            const unsigned long mid = qsv_stub_launches;
            EXPECT(qsv_layer_adjoint(first, second, n, all.data(), m.data(), v.data(), &passes) == QSV_EINVAL);
            EXPECT(qsv_layer_adjoint(second, first, n, all.data(), m.data(), v.data(), &passes) == QSV_EINVAL);
            EXPECT(qsv_stub_launches == mid && v[0] == 7.0);
            EXPECT(qsv_layer_transition(first, second, n, all.data(), v.data(), &passes) == QSV_OK);      // read-only: memory may meet
            EXPECT(passes == model_passes(n, all) && v[0] == 0.0);
            EXPECT(qsv_destroy(first) == QSV_OK);
            EXPECT(qsv_destroy(second) == QSV_OK);
            EXPECT(qsv_destroy(smaller) == QSV_OK);
            EXPECT(qsv_destroy(elsewhere) == QSV_OK);
            qsv_stub_devices = 1;
        }
        for (const std::vector<int> &qubits : lists(n)) expect_valid(psi, lambda, n, qubits);
        EXPECT(qsv_destroy(psi) == QSV_OK);
        EXPECT(qsv_destroy(lambda) == QSV_OK);
    }
    munmap(range, reserve);
    // ---- deferring registers: a refused call leaves both queues alone, a valid one flushes both first ---------------------------
    {
        const int n = 14;
        qsv_state *psi = nullptr, *lambda = nullptr, *smaller = nullptr, *elsewhere = nullptr;
        EXPECT(qsv_create(n, 0, &psi) == QSV_OK);
        EXPECT(qsv_create(n, 0, &lambda) == QSV_OK);
        EXPECT(qsv_create(n - 1, 0, &smaller) == QSV_OK);
        qsv_stub_devices = 2;
        EXPECT(qsv_create(n, 1, &elsewhere) == QSV_OK);
        EXPECT(qsv_set_option(psi, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_set_option(lambda, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_apply_1q(psi, 3, h) == QSV_OK);
        EXPECT(qsv_apply_1q(lambda, 4, h) == QSV_OK);
        const Stats queued = stats_of(psi);
        EXPECT(queued.queued == 1 && queued.launched == 0);
        expect_refusals(psi, lambda, smaller, modes, elsewhere, n);
        const std::vector<int> all = all_qubits(n);
        const std::vector<double> m = matrices(n);
        std::vector<double> v(static_cast<size_t>(n) * 8, 7.0);
        uint64_t passes = 99;
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_layer_adjoint(psi, lambda, n, all.data(), m.data(), v.data(), &passes) == QSV_OK);
        EXPECT(stats_of(psi).launched == 1 && stats_of(lambda).launched == 1);     // both queued gates went out; the walk was never queued
        EXPECT(passes == 2 && passes == model_passes(n, all) && qsv_stub_launches == before + 2 + passes);
        EXPECT(qsv_apply_1q(psi, 5, h) == QSV_OK);
        EXPECT(qsv_apply_1q(lambda, 6, h) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_layer_transition(lambda, psi, n, all.data(), v.data(), &passes) == QSV_OK);
        EXPECT(stats_of(psi).launched == 2 && stats_of(lambda).launched == 2 && qsv_stub_launches == before + 2 + passes);
        EXPECT(qsv_apply_1q(psi, 7, h) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_layer_transition(psi, psi, n, all.data(), v.data(), &passes) == QSV_OK);            // one register: one flush
        EXPECT(stats_of(psi).launched == 3 && qsv_stub_launches == before + 1 + passes);
        EXPECT(qsv_destroy(psi) == QSV_OK);
        EXPECT(qsv_destroy(lambda) == QSV_OK);
        EXPECT(qsv_destroy(smaller) == QSV_OK);
        EXPECT(qsv_destroy(elsewhere) == QSV_OK);
        qsv_stub_devices = 1;
    }
    EXPECT(qsv_destroy(modes) == QSV_OK);
    return finish("layer_adjoint");
}

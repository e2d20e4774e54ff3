// TEST INFRASTRUCTURE: drives the host side of qsv_ensemble_inner, qsv_ensemble_apply_diag_mul,
// qsv_ensemble_pauli_rotations_adjoint and qsv_ensemble_diag_phase_adjoint -- every validation branch, the planner on
// member-local masks, the angle table, the workspace, the launch of every pass with its per-member sum, and the host's copy --
// under ASan + UBSan against hip_stub.cpp (device memory is zeroed host memory and kernels do not run, so every value comes
// back 0).
// THE RULE: a valid walk launches the passes of qsv_apply_pauli_rotations' plan on one member (csrc/qsv_pauli_rotation_plan.h,
// included here as the library includes it) plus one sum per pass, whatever the number of members; the inner product and the
// cost-phase walk launch one pass and one sum; n_terms = 0 launches nothing.
// Walks: every refusal of the four calls -- null pointers, a view, member_qubits out of range, a qubit >= member_qubits or
// repeated, bad letters, offsets and lengths, angles and gammas that are not finite, registers of different sizes and devices,
// the same register twice (accepted by the inner product and by diag_mul), a diagonal of another size or device, a mode
// register, a change of the member size while the ensemble log holds steps -- each before any launch and with qsv_defer_stats
// of both registers unchanged, on plain and deferring registers; then valid calls for members of 1 .. 20 qubits as 1 .. 4096
// members.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <limits>
#include <string>
#include <vector>

#include "driver_common.h"
#include "qsv_pauli_rotation_plan.h"

struct List {
    std::vector<int> offsets{0}, qubits;
    std::string letters;
    int count = 0;
    void add(const std::string &paulis, const std::vector<int> &qs) {
        letters += paulis;
        qubits.insert(qubits.end(), qs.begin(), qs.end());
        offsets.push_back(static_cast<int>(qubits.size()));
        ++count;
    }
};

static uint64_t model_passes(int n, const List &l) {
    std::vector<qsv_pauli_plan::Term> terms(static_cast<size_t>(l.count));
    for (int t = 0; t < l.count; ++t)
        for (int j = l.offsets[t]; j < l.offsets[t + 1]; ++j) {
            const uint64_t bit = 1ull << (n - 1 - l.qubits[j]);
            const char c = l.letters[j];
            if (c == 'X' || c == 'Y') terms[t].xmask |= bit;
            if (c == 'Z' || c == 'Y') terms[t].zmask |= bit;
        }
    return qsv_pauli_rotation_plan::plan(terms).size();
}

// the diagonal, a flipping group of eight with a ninth behind it, the identity string, pivots on bit 0 and on the top bit,
// strings of full weight
static List walk_list(int n) {
    List l;
    const int a = 0, b = n - 1;
    l.add("Z", {a});
    l.add("", {});
    if (n >= 2) {
        for (const char *s : {"XX", "ZZ", "YY", "XY", "YX", "XX", "YY", "XY", "YX", "XX"}) l.add(s, {a, b});
    }
    l.add("X", {b});
    l.add("Y", {a});
    l.add("I", {a});
    std::vector<int> all(n);
    std::string full, zs;
    for (int q = 0; q < n; ++q) {
        all[q] = q;
        full += "XYZ"[q % 3];
        zs += 'Z';
    }
    l.add(full, all);
    l.add(zs, all);
    l.add("Z", {b});
    return l;
}

static std::vector<double> angles(uint64_t members, int count) {
    std::vector<double> t(static_cast<size_t>(members) * count);
    for (size_t i = 0; i < t.size(); ++i) t[i] = 0.001 * static_cast<double>(i % 3001) - 1.5;
    return t;
}

static void expect_valid(qsv_state *psi, qsv_state *lambda, qsv_diag *d, int n, uint64_t members) {
    const List l = walk_list(n);
    const std::vector<double> thetas = angles(members, l.count), gammas = angles(members, 1);
    std::vector<double> values(static_cast<size_t>(members) * l.count * 2, 7.0);
    uint64_t passes = 99;
    unsigned long before = qsv_stub_launches;
    EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), thetas.data(),
                                                values.data(), &passes) == QSV_OK);
    EXPECT(passes == model_passes(n, l) && passes >= (n >= 2 ? 3u : 1u) && qsv_stub_launches - before == 2 * passes);     // a pass and its sum
    for (double v : values) EXPECT(v == 0.0);          // every value was written
    uint64_t forward = 98;
    EXPECT(qsv_ensemble_apply_pauli_rotations(psi, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), thetas.data(), &forward) == QSV_OK);
    EXPECT(forward == passes);
    EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), thetas.data(),
                                                values.data(), nullptr) == QSV_OK);
    // n_terms = 0: nothing happens, no array needed
    before = qsv_stub_launches;
    passes = 99;
    EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
    EXPECT(qsv_stub_launches == before);
    std::vector<double> pair(static_cast<size_t>(members) * 2, 7.0);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d, gammas.data(), pair.data()) == QSV_OK);
    EXPECT(qsv_stub_launches - before == 2);
    for (double v : pair) EXPECT(v == 0.0);
    for (qsv_state *b : {lambda, psi}) {               // a may be b
        std::fill(pair.begin(), pair.end(), 7.0);
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_inner(psi, b, n, pair.data()) == QSV_OK);
        EXPECT(qsv_stub_launches - before == 2);
        for (double v : pair) EXPECT(v == 0.0);
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_diag_mul(b, psi, n, d) == QSV_OK);          // dst may be src
        EXPECT(qsv_stub_launches - before == 1);
    }
}

// every refusal on two registers of n_total qubits read as members of n >= 3 qubits; nothing is launched or flushed
static void expect_refusals(qsv_state *psi, qsv_state *lambda, qsv_state *smaller, qsv_state *modes, qsv_state *elsewhere, qsv_state *view, qsv_diag *d,
                            qsv_diag *d_wide, qsv_diag *d_elsewhere, int n_total, int n) {
    const uint64_t members = 1ull << (n_total - n);
    const List l = walk_list(n);
    const std::vector<double> thetas = angles(members, l.count), gammas = angles(members, 1);
    std::vector<double> nan = thetas, inf = thetas, gnan = gammas, values(static_cast<size_t>(members) * l.count * 2, 7.0);
    nan[thetas.size() - 1] = std::numeric_limits<double>::quiet_NaN();
    inf[l.count] = std::numeric_limits<double>::infinity();
    gnan[members - 1] = std::numeric_limits<double>::quiet_NaN();
    const int one[2] = {0, 1}, two[2] = {0, 2}, down[3] = {0, 1, 0}, below[2] = {-1, 0}, longer[2] = {0, 65};
    const int out_of_range[1] = {n}, negative[1] = {-1}, twice[2] = {1, 1};
    const std::vector<int> many(65, 0);
    const std::string xs(65, 'X');
    uint64_t passes = 99;
    const Stats stats_psi = stats_of(psi), stats_lambda = stats_of(lambda);
    const unsigned long before = qsv_stub_launches;
    double *v = values.data();
    const double *th = thetas.data();
    auto walk = [&](qsv_state *a, qsv_state *b, int mq, int count, const int *offsets, const int *qubits, const char *letters, const double *angle, double *out) {
        return qsv_ensemble_pauli_rotations_adjoint(a, b, mq, count, offsets, qubits, letters, angle, out, &passes);
    };
    EXPECT(walk(nullptr, lambda, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, nullptr, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, nullptr, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, nullptr, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, one, nullptr, th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, one, "X", nullptr, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, one, "X", th, nullptr) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, -1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(view, lambda, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, view, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, -1, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n_total + 1, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, out_of_range, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, negative, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, two, twice, "XX", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, one, one, "Q", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 2, down, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, below, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, 1, longer, many.data(), xs.c_str(), th, v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), nan.data(), v) == QSV_EINVAL);
    EXPECT(walk(psi, lambda, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), inf.data(), v) == QSV_EINVAL);
    EXPECT(walk(psi, smaller, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(smaller, psi, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, elsewhere, n, 1, one, one, "X", th, v) == QSV_EINVAL);
    EXPECT(walk(psi, psi, n, 1, one, one, "X", th, v) == QSV_EINVAL);          // the same handle: the memory meets
    EXPECT(walk(psi, modes, n, 1, one, one, "X", th, v) == QSV_ESTATE);
    EXPECT(walk(modes, psi, n, 1, one, one, "X", th, v) == QSV_ESTATE);
    const double *g = gammas.data();
    EXPECT(qsv_ensemble_diag_phase_adjoint(nullptr, lambda, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, nullptr, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, nullptr, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d, nullptr, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d, g, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(view, lambda, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, view, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, -1, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n_total + 1, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n + 1, d, g, v) == QSV_EINVAL);       // the diagonal has n qubits
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d_wide, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d_elsewhere, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, d, gnan.data(), v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, smaller, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, elsewhere, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, psi, n, d, g, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_diag_phase_adjoint(psi, modes, n, d, g, v) == QSV_ESTATE);
    EXPECT(qsv_ensemble_diag_phase_adjoint(modes, psi, n, d, g, v) == QSV_ESTATE);
    EXPECT(qsv_ensemble_inner(nullptr, lambda, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, nullptr, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, lambda, n, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(view, lambda, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, view, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, lambda, -1, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, lambda, n_total + 1, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, smaller, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, elsewhere, n, v) == QSV_EINVAL);
    EXPECT(qsv_ensemble_inner(psi, modes, n, v) == QSV_ESTATE);
    EXPECT(qsv_ensemble_inner(modes, modes, n, v) == QSV_ESTATE);
    EXPECT(qsv_ensemble_apply_diag_mul(nullptr, psi, n, d) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(lambda, nullptr, n, d) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(lambda, psi, n, nullptr) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(view, psi, n, d) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(lambda, psi, n, d_wide) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(lambda, psi, n, d_elsewhere) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(smaller, psi, n, d) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(elsewhere, psi, n, d) == QSV_EINVAL);
    EXPECT(qsv_ensemble_apply_diag_mul(modes, psi, n, d) == QSV_ESTATE);
    for (double x : values) EXPECT(x == 7.0);          // a refused call writes no value
    const Stats now_psi = stats_of(psi), now_lambda = stats_of(lambda);
    EXPECT(now_psi.queued == stats_psi.queued && now_psi.launched == stats_psi.launched);
    EXPECT(now_lambda.queued == stats_lambda.queued && now_lambda.launched == stats_lambda.launched);
    EXPECT(qsv_stub_launches == before);
}

struct Others {
    qsv_state *smaller = nullptr, *elsewhere = nullptr, *view = nullptr, *modes = nullptr;
    qsv_diag *d = nullptr, *d_wide = nullptr, *d_elsewhere = nullptr;
    std::vector<double> mem;
    Others(int n_total, int n) : mem(size_t{2} << n_total, 0.0) {
        EXPECT(qsv_create_qudit(3, 3, 0, &modes) == QSV_OK);
        EXPECT(qsv_create(n_total - 1, 0, &smaller) == QSV_OK);
        qsv_stub_devices = 2;
        EXPECT(qsv_create(n_total, 1, &elsewhere) == QSV_OK);
        EXPECT(qsv_diag_create(n, 1, &d_elsewhere) == QSV_OK);
        EXPECT(qsv_create_view(n_total, 0, mem.data(), 1ull << n_total, nullptr, &view) == QSV_OK);
        EXPECT(qsv_diag_create(n, 0, &d) == QSV_OK);
        EXPECT(qsv_diag_create(n_total, 0, &d_wide) == QSV_OK);
    }
    ~Others() {
        EXPECT(qsv_destroy(smaller) == QSV_OK);
        EXPECT(qsv_destroy(elsewhere) == QSV_OK);
        EXPECT(qsv_destroy(view) == QSV_OK);
        EXPECT(qsv_destroy(modes) == QSV_OK);
        EXPECT(qsv_diag_destroy(d) == QSV_OK);
        EXPECT(qsv_diag_destroy(d_wide) == QSV_OK);
        EXPECT(qsv_diag_destroy(d_elsewhere) == QSV_OK);
        qsv_stub_devices = 1;
    }
};

int main() {
    // ---- valid calls: members of 1 .. 20 qubits as 1 .. 4096 members ----------------------------------------------------------------
    for (int n = 1; n <= 20; ++n)
        for (int b : {0, 1, 3, 6, 12}) {
            if (n + b > 20 && !(n == 8 && b == 12)) continue;
            qsv_state *psi = nullptr, *lambda = nullptr;
            qsv_diag *d = nullptr;
            EXPECT(qsv_create(n + b, 0, &psi) == QSV_OK);
            EXPECT(qsv_create(n + b, 0, &lambda) == QSV_OK);
            EXPECT(qsv_diag_create(n, 0, &d) == QSV_OK);
            for (int cap : {0, 2}) {
                EXPECT(qsv_set_option(psi, QSV_OPT_GRID_CAP, cap) == QSV_OK);
                expect_valid(psi, lambda, d, n, 1ull << b);
            }
            EXPECT(qsv_destroy(psi) == QSV_OK);
            EXPECT(qsv_destroy(lambda) == QSV_OK);
            EXPECT(qsv_diag_destroy(d) == QSV_OK);
        }
    // ---- refusals on plain registers, and the member size against the ensemble log --------------------------------------------------
    for (int n : {3, 10}) {
        const int n_total = n + 3;
        Others o(n_total, n);
        qsv_state *psi = nullptr, *lambda = nullptr;
        EXPECT(qsv_create(n_total, 0, &psi) == QSV_OK);
        EXPECT(qsv_create(n_total, 0, &lambda) == QSV_OK);
        expect_refusals(psi, lambda, o.smaller, o.modes, o.elsewhere, o.view, o.d, o.d_wide, o.d_elsewhere, n_total, n);
        // one step in psi's ensemble log: the same member size goes on, another is refused until the log is read
        qsv_channel *ad = nullptr;
        EXPECT(qsv_channel_create(1, 2, amplitude_damping(0.3).data(), 0, &ad) == QSV_OK);
        const std::vector<double> u(8, 0.5), thetas = angles(16, 1);
        const int q = 0, offsets[2] = {0, 1};
        std::vector<double> values(64, 7.0);
        uint64_t passes = 99, steps = 0;
        EXPECT(qsv_ensemble_apply_channel(psi, n, ad, &q, u.data(), nullptr) == QSV_OK);
        EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n, 1, offsets, &q, "X", thetas.data(), values.data(), &passes) == QSV_OK && passes == 1);
        EXPECT(qsv_ensemble_inner(psi, lambda, n, values.data()) == QSV_OK);
        EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, o.d, thetas.data(), values.data()) == QSV_OK);
        const unsigned long before = qsv_stub_launches;
        std::fill(values.begin(), values.end(), 7.0);
        EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n - 1, 1, offsets, &q, "X", thetas.data(), values.data(), &passes) == QSV_ESTATE);
        EXPECT(qsv_ensemble_inner(psi, lambda, n - 1, values.data()) == QSV_ESTATE);
        EXPECT(qsv_ensemble_inner(lambda, psi, n - 1, values.data()) == QSV_OK);         // the log is psi's: lambda's workspace is free to change
        EXPECT(qsv_stub_launches == before + 2);
        EXPECT(qsv_ensemble_log_read(psi, nullptr, nullptr, 0, &steps) == QSV_OK && steps == 1);
        std::vector<int32_t> branches(8);
        std::vector<double> probs(8);
        EXPECT(qsv_ensemble_log_read(psi, branches.data(), probs.data(), 1, &steps) == QSV_OK);
        EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n - 1, 1, offsets, &q, "X", thetas.data(), values.data(), &passes) == QSV_OK);
        EXPECT(qsv_channel_destroy(ad) == QSV_OK);
        EXPECT(qsv_destroy(psi) == QSV_OK);
        EXPECT(qsv_destroy(lambda) == QSV_OK);
    }
    // ---- deferring registers: a refused call leaves both queues alone, a valid one flushes both first ---------------------------
    {
        const int n = 11, n_total = 14;
        Others o(n_total, n);
        qsv_state *psi = nullptr, *lambda = nullptr;
        EXPECT(qsv_create(n_total, 0, &psi) == QSV_OK);
        EXPECT(qsv_create(n_total, 0, &lambda) == QSV_OK);
        EXPECT(qsv_set_option(psi, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_set_option(lambda, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        auto queue_one = [&]() {
            EXPECT(qsv_apply_1q(psi, 5, h) == QSV_OK);
            EXPECT(qsv_apply_1q(lambda, 6, h) == QSV_OK);
        };
        queue_one();
        EXPECT(stats_of(psi).queued == 1 && stats_of(psi).launched == 0 && stats_of(lambda).queued == 1 && stats_of(lambda).launched == 0);
        expect_refusals(psi, lambda, o.smaller, o.modes, o.elsewhere, o.view, o.d, o.d_wide, o.d_elsewhere, n_total, n);
        const List l = walk_list(n);
        const std::vector<double> thetas = angles(8, l.count);
        std::vector<double> values(static_cast<size_t>(8) * l.count * 2, 7.0);
        uint64_t passes = 99;
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_ensemble_pauli_rotations_adjoint(psi, lambda, n, l.count, l.offsets.data(), l.qubits.data(), l.letters.c_str(), thetas.data(),
                                                    values.data(), &passes) == QSV_OK);
        EXPECT(stats_of(psi).launched == 1 && stats_of(lambda).launched == 1);     // both queued gates went out; the walk was never queued
        EXPECT(passes == model_passes(n, l) && qsv_stub_launches == before + 2 + 2 * passes);
        queue_one();
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_diag_phase_adjoint(psi, lambda, n, o.d, thetas.data(), values.data()) == QSV_OK);
        EXPECT(stats_of(psi).launched == 2 && stats_of(lambda).launched == 2 && qsv_stub_launches == before + 2 + 2);
        queue_one();
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_inner(psi, lambda, n, values.data()) == QSV_OK);
        EXPECT(stats_of(psi).launched == 3 && stats_of(lambda).launched == 3 && qsv_stub_launches == before + 2 + 2);
        queue_one();
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_apply_diag_mul(lambda, psi, n, o.d) == QSV_OK);
        EXPECT(stats_of(psi).launched == 4 && stats_of(lambda).launched == 4 && qsv_stub_launches == before + 2 + 1);
        EXPECT(qsv_apply_1q(psi, 7, h) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_ensemble_inner(psi, psi, n, values.data()) == QSV_OK);            // one register: one flush
        EXPECT(stats_of(psi).launched == 5 && qsv_stub_launches == before + 1 + 2);
        EXPECT(qsv_destroy(psi) == QSV_OK);
        EXPECT(qsv_destroy(lambda) == QSV_OK);
    }
    return finish("ensemble_adjoint");
}

// TEST INFRASTRUCTURE: drives the host side of qsv_apply_pauli_sum, qsv_pauli_transition_sum and
// qsv_pauli_rotations_adjoint -- every refusal, the parsing of the flattened term list, both planners, the argument
// builders, the slicing of the scratch buffer and the launch of every pass -- under ASan + UBSan against hip_stub.cpp
// (device memory is zeroed host memory and kernels do not run).  The number of launches of every valid call is compared
// with models of the two grouping rules written here on the letters themselves.
// Walks: null handles and pointers, a negative count, decreasing offsets, a term of 65 letters, repeated and out-of-range
// qubits, a bad letter, the same register twice, overlapping views, registers of different sizes, a destination that is too
// small, mode registers -- each refused before any launch and with both deferred queues left alone -- and then valid lists
// on registers of 1 to 18 qubits and on views.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "driver_common.h"

struct Terms {
    std::vector<int> offsets = {0}, qubits;
    std::string letters;
    std::vector<double> coeffs, thetas;    // coeffs: interleaved complex
    void add(const std::string &paulis, const std::vector<int> &qs) {
        letters += paulis;
        qubits.insert(qubits.end(), qs.begin(), qs.end());
        offsets.push_back(static_cast<int>(qubits.size()));
        thetas.push_back(0.125 * static_cast<double>(thetas.size() % 9) - 0.5);
        coeffs.push_back(1.0 + 0.25 * static_cast<double>(thetas.size() % 5));
        coeffs.push_back(0.5 - 0.125 * static_cast<double>(thetas.size() % 3));
    }
    int count() const { return static_cast<int>(thetas.size()); }
    uint64_t flips(int t) const {
        uint64_t f = 0;
        for (int j = offsets[t]; j < offsets[t + 1]; ++j)
            if (std::strchr("XxYy", letters[j])) f |= 1ull << qubits[j];
        return f;
    }
    // the sum's rule: terms that flip the same qubits form a group, a group is cut into passes of 8
    uint64_t sum_passes() const {
        std::map<uint64_t, int> members;
        for (int t = 0; t < count(); ++t) ++members[flips(t)];
        uint64_t passes = 0;
        for (const auto &group : members) passes += static_cast<uint64_t>((group.second + 7) / 8);
        return passes;
    }
    // the rotations' greedy rule: a term joins the open pass if the pass holds fewer than 8 terms and the term flips
    // nothing, the pass flips nothing yet, or both flip the same qubits
    uint64_t walk_passes() const {
        uint64_t passes = 0, open_flips = 0;
        int held = 0;
        for (int t = 0; t < count(); ++t) {
            const uint64_t f = flips(t);
            if (passes == 0 || held == 8 || !(f == 0 || open_flips == 0 || f == open_flips)) {
                ++passes;
                held = 0;
                open_flips = 0;
            }
            if (open_flips == 0) open_flips = f;
            ++held;
        }
        return passes;
    }
};

static int apply(qsv_state *dst, qsv_state *src, const Terms &t, int accumulate, uint64_t *passes) {
    return qsv_apply_pauli_sum(dst, src, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), t.coeffs.data(), accumulate, passes);
}
static int transition(qsv_state *bra, qsv_state *ket, const Terms &t, double *values, double *re, double *im, uint64_t *passes) {
    return qsv_pauli_transition_sum(bra, ket, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), t.coeffs.data(), values, re, im, passes);
}
static int adjoint(qsv_state *psi, qsv_state *lambda, const Terms &t, double *values, uint64_t *passes) {
    return qsv_pauli_rotations_adjoint(psi, lambda, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), t.thetas.data(), values, passes);
}

// every entry point on a valid list: status, reported passes and launches made against the models
static void expect_valid(qsv_state *a, qsv_state *b, const Terms &t) {
    std::vector<double> values(2 * static_cast<size_t>(t.count()) + 2, 7.0);
    double re = 7.0, im = 7.0;
    for (int accumulate : {0, 1}) {
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(apply(a, b, t, accumulate, &passes) == QSV_OK);
        EXPECT(passes == t.sum_passes() && qsv_stub_launches - before == passes);
        EXPECT(apply(b, a, t, accumulate, nullptr) == QSV_OK);
    }
    for (qsv_state *ket : {b, a}) {                                    // two registers, and bra == ket
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(transition(a, ket, t, values.data(), &re, &im, &passes) == QSV_OK);
        EXPECT(passes == t.sum_passes() && qsv_stub_launches - before == passes);
        EXPECT(re == 0.0 && im == 0.0 && values[2 * static_cast<size_t>(t.count())] == 7.0);     // zeroed memory in, zeros out; no write past the end
        EXPECT(transition(a, ket, t, nullptr, &re, &im, nullptr) == QSV_OK);
        EXPECT(qsv_pauli_transition_sum(a, ket, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), nullptr, nullptr, &re, &im, nullptr) == QSV_OK);
    }
    {
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(adjoint(a, b, t, values.data(), &passes) == QSV_OK);
        EXPECT(passes == t.walk_passes() && qsv_stub_launches - before == passes);
        EXPECT(values[2 * static_cast<size_t>(t.count())] == 7.0);
        EXPECT(adjoint(b, a, t, values.data(), nullptr) == QSV_OK);
    }
}

// every refusal of the three calls on the pair (a, b); nothing may be launched
static void expect_refusals(qsv_state *a, qsv_state *b, int n) {
    Terms one;
    one.add("Z", {0});
    double values[4] = {0, 0, 0, 0}, re = 0, im = 0;
    uint64_t passes = 99;
    const unsigned long before = qsv_stub_launches;
    const int *off = one.offsets.data(), *qs = one.qubits.data();
    const char *letters = one.letters.data();
    const double *c = one.coeffs.data(), *th = one.thetas.data();
    // ---- null pointers, negative counts ---------------------------------------------------------------------------------
    EXPECT(apply(nullptr, b, one, 0, nullptr) == QSV_EINVAL);
    EXPECT(apply(a, nullptr, one, 0, nullptr) == QSV_EINVAL);
    EXPECT(qsv_apply_pauli_sum(a, b, 1, nullptr, qs, letters, c, 0, nullptr) == QSV_EINVAL);
    EXPECT(qsv_apply_pauli_sum(a, b, 1, off, nullptr, letters, c, 0, nullptr) == QSV_EINVAL);
    EXPECT(qsv_apply_pauli_sum(a, b, 1, off, qs, nullptr, c, 0, nullptr) == QSV_EINVAL);
    EXPECT(qsv_apply_pauli_sum(a, b, 1, off, qs, letters, nullptr, 0, nullptr) == QSV_EINVAL);
    EXPECT(qsv_apply_pauli_sum(a, b, -1, off, qs, letters, c, 0, nullptr) == QSV_EINVAL);
    EXPECT(transition(nullptr, b, one, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(transition(a, nullptr, one, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(transition(a, b, one, values, nullptr, &im, nullptr) == QSV_EINVAL);
    EXPECT(transition(a, b, one, values, &re, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_transition_sum(a, b, 1, nullptr, qs, letters, c, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_transition_sum(a, b, 1, off, nullptr, letters, c, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_transition_sum(a, b, 1, off, qs, nullptr, c, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_transition_sum(a, b, -1, off, qs, letters, c, values, &re, &im, nullptr) == QSV_EINVAL);
    EXPECT(adjoint(nullptr, b, one, values, nullptr) == QSV_EINVAL);
    EXPECT(adjoint(a, nullptr, one, values, nullptr) == QSV_EINVAL);
    EXPECT(adjoint(a, b, one, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, nullptr, qs, letters, th, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, off, nullptr, letters, th, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, off, qs, nullptr, th, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, off, qs, letters, nullptr, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_pauli_rotations_adjoint(a, b, -1, off, qs, letters, th, values, nullptr) == QSV_EINVAL);
    // ---- the same register twice ------------------------------------------------------------------------------------------
    EXPECT(apply(a, a, one, 0, nullptr) == QSV_EINVAL);
    EXPECT(apply(a, a, one, 1, nullptr) == QSV_EINVAL);
    EXPECT(adjoint(a, a, one, values, nullptr) == QSV_EINVAL);
    // ---- offsets: decreasing, negative start, a term of 65 letters --------------------------------------------------------
    {
        const int down[3] = {0, 1, 0}, negative[2] = {-1, 0}, wide[2] = {0, 65};
        const int two[2] = {0, 0};
        const double four[4] = {0.1, 0.2, 0.3, 0.4};
        std::vector<int> many(65);
        for (int j = 0; j < 65; ++j) many[j] = j;
        const std::string zs(65, 'Z');
        double out[4];
        EXPECT(qsv_apply_pauli_sum(a, b, 2, down, two, "ZZ", four, 0, nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_sum(a, b, 1, negative, two, "ZZ", four, 0, nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_sum(a, b, 1, wide, many.data(), zs.data(), four, 0, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_transition_sum(a, b, 2, down, two, "ZZ", four, out, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_transition_sum(a, b, 1, negative, two, "ZZ", four, out, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_transition_sum(a, b, 1, wide, many.data(), zs.data(), four, out, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_rotations_adjoint(a, b, 2, down, two, "ZZ", four, out, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, negative, two, "ZZ", four, out, nullptr) == QSV_EINVAL);
        EXPECT(qsv_pauli_rotations_adjoint(a, b, 1, wide, many.data(), zs.data(), four, out, nullptr) == QSV_EINVAL);
    }
    // ---- a bad term anywhere in the list stops the call ----------------------------------------------------------------------
    for (int bad = 0; bad < 4; ++bad) {
        Terms t;
        t.add("Z", {0});
        t.add("x", {n - 1});
        if (bad == 0) t.add("Q", {0});                             // a bad letter
        if (bad == 1) t.add("ZZ", {0, 0});                         // a repeated qubit
        if (bad == 2) t.add("Z", {n});                             // out of range
        if (bad == 3) t.add("Z", {-1});
        double out[6];
        EXPECT(apply(a, b, t, 0, &passes) == QSV_EINVAL);
        EXPECT(apply(a, b, t, 1, &passes) == QSV_EINVAL);
        EXPECT(transition(a, b, t, out, &re, &im, &passes) == QSV_EINVAL);
        EXPECT(adjoint(a, b, t, out, &passes) == QSV_EINVAL);
    }
    EXPECT(qsv_stub_launches == before);
}

int main() {
    for (int n : {1, 2, 3, 6, 7, 13, 14, 18}) {
        qsv_state *a = nullptr, *b = nullptr;
        EXPECT(qsv_create(n, 0, &a) == QSV_OK);
        EXPECT(qsv_create(n, 0, &b) == QSV_OK);
        uint64_t passes = 99;
        double re = 7.0, im = 7.0;
        // ---- the empty list: no pointer needed; the overwriting sum zeroes dst without a kernel ----------------------------
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_pauli_sum(a, b, 0, nullptr, nullptr, nullptr, nullptr, 0, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_apply_pauli_sum(a, b, 0, nullptr, nullptr, nullptr, nullptr, 1, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_pauli_transition_sum(a, b, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &re, &im, &passes) == QSV_OK && passes == 0);
        EXPECT(re == 0.0 && im == 0.0);
        EXPECT(qsv_pauli_rotations_adjoint(a, b, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
        EXPECT(qsv_stub_launches == before);
        expect_refusals(a, b, n);
        // ---- valid lists: identity and empty terms, every qubit as the pivot, diagonal terms in between ------------------------
        {
            Terms t;
            t.add("", {});
            t.add("I", {0});
            t.add("i", {n - 1});
            for (int q = 0; q < n; ++q) {
                t.add("X", {q});
                t.add("y", {q});
                t.add("z", {q});
                if (q + 1 < n) {
                    t.add("XX", {q, q + 1});
                    t.add("YY", {q + 1, q});
                    t.add("ZZ", {q, q + 1});
                    t.add("Zx", {q, q + 1});
                }
            }
            expect_valid(a, b, t);
        }
        for (int count : {1, 7, 8, 9, 16, 17, 25, 40, 100}) {
            Terms shared, diagonal, alternating;
            for (int j = 0; j < count; ++j) {
                if (n >= 2) shared.add(j % 2 ? "XZ" : "YI", {0, 1 + j % (n - 1)});
                else shared.add(j % 2 ? "X" : "y", {0});
                diagonal.add(j % 3 ? "Z" : "I", {j % n});
                alternating.add(j % 2 ? "X" : "Y", {j % 2 ? 0 : n - 1});
            }
            expect_valid(a, b, shared);
            expect_valid(a, b, diagonal);
            expect_valid(a, b, alternating);
            EXPECT(shared.sum_passes() == static_cast<uint64_t>((count + 7) / 8) && shared.walk_passes() == shared.sum_passes());
            EXPECT(diagonal.sum_passes() == static_cast<uint64_t>((count + 7) / 8));
            if (n >= 2) EXPECT(alternating.walk_passes() == static_cast<uint64_t>(count) && alternating.sum_passes() == static_cast<uint64_t>((count / 2 + 7) / 8 + (count - count / 2 + 7) / 8));
        }
        // ---- sizes: a smaller destination takes the source's size if it has the room; accumulating needs equal sizes -------------
        if (n >= 2) {
            qsv_state *small = nullptr;
            EXPECT(qsv_create(n - 1, 0, &small) == QSV_OK);
            Terms t;
            t.add("X", {0});
            double out[2];
            before = qsv_stub_launches;
            EXPECT(apply(small, a, t, 0, nullptr) == QSV_ENOMEM);
            EXPECT(apply(a, small, t, 1, nullptr) == QSV_EINVAL);
            EXPECT(transition(a, small, t, out, &re, &im, nullptr) == QSV_EINVAL);
            EXPECT(adjoint(a, small, t, out, nullptr) == QSV_EINVAL);
            EXPECT(adjoint(small, a, t, out, nullptr) == QSV_EINVAL);
            EXPECT(qsv_stub_launches == before);
            int qubits = 0;
            EXPECT(apply(a, small, t, 0, nullptr) == QSV_OK);          // a shrinks to small's size ...
            EXPECT(qsv_num_qubits(a, &qubits) == QSV_OK && qubits == n - 1);
            EXPECT(apply(a, b, t, 0, nullptr) == QSV_OK);              // ... and grows back inside its allocation
            EXPECT(qsv_num_qubits(a, &qubits) == QSV_OK && qubits == n);
            EXPECT(qsv_destroy(small) == QSV_OK);
        }
        EXPECT(qsv_destroy(a) == QSV_OK);
        EXPECT(qsv_destroy(b) == QSV_OK);
    }
    // ---- deferring registers: a refused call leaves both queues alone, a valid one flushes both first -------------------------
    for (int call = 0; call < 3; ++call) {
        qsv_state *a = nullptr, *b = nullptr;
        EXPECT(qsv_create(13, 0, &a) == QSV_OK);
        EXPECT(qsv_create(13, 0, &b) == QSV_OK);
        EXPECT(qsv_set_option(a, QSV_OPT_DEFER, 2) == QSV_OK);
        EXPECT(qsv_set_option(b, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_apply_1q(a, 3, h) == QSV_OK);
        EXPECT(qsv_apply_1q(b, 5, h) == QSV_OK);
        uint64_t queued_a = 0, queued_b = 0, launched_a = 0, launched_b = 0, after = 0, launched = 0;
        EXPECT(qsv_defer_stats(a, &queued_a, &launched_a) == QSV_OK);
        EXPECT(qsv_defer_stats(b, &queued_b, &launched_b) == QSV_OK);
        const unsigned long before = qsv_stub_launches;
        Terms bad, good;
        bad.add("X", {13});
        good.add("X", {12});
        double out[2], re = 0, im = 0;
        const auto run = [&](const Terms &t) {
            return call == 0 ? apply(a, b, t, 1, nullptr) : call == 1 ? transition(a, b, t, out, &re, &im, nullptr) : adjoint(a, b, t, out, nullptr);
        };
        EXPECT(run(bad) == QSV_EINVAL);
        EXPECT(qsv_defer_stats(a, &after, &launched) == QSV_OK && after == queued_a && launched == launched_a);
        EXPECT(qsv_defer_stats(b, &after, &launched) == QSV_OK && after == queued_b && launched == launched_b);
        EXPECT(queued_a == 1 && queued_b == 1 && qsv_stub_launches == before);
        EXPECT(run(good) == QSV_OK);
        EXPECT(qsv_defer_stats(a, &after, &launched) == QSV_OK && after == 1 && launched == launched_a + 1);     // the queued gates went out;
        EXPECT(qsv_defer_stats(b, &after, &launched) == QSV_OK && after == 1 && launched == launched_b + 1);     // the call itself was never queued
        EXPECT(qsv_stub_launches == before + 3);
        EXPECT(qsv_destroy(a) == QSV_OK);
        EXPECT(qsv_destroy(b) == QSV_OK);
    }
    // ---- views on caller-owned memory: overlapping windows are refused, disjoint ones work; mode registers are refused --------
    {
        std::vector<double> mem(2 * 160, 0.0);
        qsv_state *low = nullptr, *mid = nullptr, *high = nullptr, *owned = nullptr;
        EXPECT(qsv_create_view(6, 0, mem.data(), 64, nullptr, &low) == QSV_OK);
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 32, 64, nullptr, &mid) == QSV_OK);       // amplitudes 32..95: meets both
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 64, 96, nullptr, &high) == QSV_OK);      // amplitudes 64..127 (room for 96)
        EXPECT(qsv_create(6, 0, &owned) == QSV_OK);
        Terms t;
        t.add("XY", {5, 0});
        t.add("ZZ", {2, 3});
        t.add("yx", {0, 5});
        t.add("XY", {4, 0});
        double out[8], re = 0, im = 0;
        const unsigned long before = qsv_stub_launches;
        EXPECT(apply(low, mid, t, 0, nullptr) == QSV_EINVAL);
        EXPECT(apply(mid, low, t, 1, nullptr) == QSV_EINVAL);
        EXPECT(apply(high, mid, t, 0, nullptr) == QSV_EINVAL);
        EXPECT(adjoint(low, mid, t, out, nullptr) == QSV_EINVAL);
        EXPECT(adjoint(mid, high, t, out, nullptr) == QSV_EINVAL);
        EXPECT(qsv_stub_launches == before);
        EXPECT(transition(low, mid, t, out, &re, &im, nullptr) == QSV_OK);                    // read-only: any two windows
        expect_valid(low, high, t);
        expect_valid(high, owned, t);
        uint64_t passes = 0;
        EXPECT(apply(low, owned, t, 0, &passes) == QSV_OK && passes == 3);
        EXPECT(adjoint(low, high, t, out, &passes) == QSV_OK && passes == 2);
        qsv_state *modes = nullptr;
        EXPECT(qsv_create_qudit(3, 3, 0, &modes) == QSV_OK);
        EXPECT(apply(modes, low, t, 0, nullptr) == QSV_ESTATE);
        EXPECT(apply(low, modes, t, 0, nullptr) == QSV_ESTATE);
        EXPECT(transition(modes, low, t, out, &re, &im, nullptr) == QSV_ESTATE);
        EXPECT(transition(low, modes, t, out, &re, &im, nullptr) == QSV_ESTATE);
        EXPECT(adjoint(modes, low, t, out, nullptr) == QSV_ESTATE);
        EXPECT(adjoint(low, modes, t, out, nullptr) == QSV_ESTATE);
        for (qsv_state *st : {low, mid, high, owned, modes}) EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("Pauli-operator");
}

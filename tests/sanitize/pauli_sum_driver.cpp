// TEST INFRASTRUCTURE: drives the host side of qsv_expect_pauli_sum -- every validation branch, the parsing of the
// flattened term list, the planner and the launch / partial-sum bookkeeping of every pass -- under ASan + UBSan against
// hip_stub.cpp (device memory is zeroed host memory and kernels do not run: every expectation value comes back 0).
// Walks: null pointers, a negative count, decreasing offsets, a term of 65 letters, repeated and out-of-range qubits, a bad
// letter -- each refused before any launch -- and then valid lists on registers of 1 to 18 qubits, on a view and on a mode
// register: parsing, planning, one launch per planned pass, the copy of the partials and their sums.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "driver_common.h"

struct Terms {
    std::vector<int> offsets = {0}, qubits;
    std::string letters;
    void add(const std::string &paulis, const std::vector<int> &qs) {
        letters += paulis;
        qubits.insert(qubits.end(), qs.begin(), qs.end());
        offsets.push_back(static_cast<int>(qubits.size()));
    }
    int count() const { return static_cast<int>(offsets.size()) - 1; }
};

static int run(qsv_state *st, const Terms &t, const double *coeffs, double *values, double *re, double *im, uint64_t *passes) {
    return qsv_expect_pauli_sum(st, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), coeffs, values, re, im, passes);
}

int main() {
    for (int n : {1, 2, 3, 6, 7, 13, 14, 18}) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        double re = 7.0, im = 7.0;
        uint64_t passes = 99;
        // ---- the empty sum: 0, no launch, no pointer besides re / im needed -------------------------------------------
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_expect_pauli_sum(st, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &re, &im, &passes) == QSV_OK);
        EXPECT(re == 0.0 && im == 0.0 && passes == 0 && qsv_stub_launches == before);
        // ---- null pointers, negative counts ---------------------------------------------------------------------------
        Terms one;
        one.add("Z", {0});
        EXPECT(run(nullptr, one, nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(run(st, one, nullptr, nullptr, nullptr, &im, nullptr) == QSV_EINVAL);
        EXPECT(run(st, one, nullptr, nullptr, &re, nullptr, nullptr) == QSV_EINVAL);
        EXPECT(qsv_expect_pauli_sum(st, 1, nullptr, one.qubits.data(), one.letters.data(), nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_expect_pauli_sum(st, 1, one.offsets.data(), nullptr, one.letters.data(), nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_expect_pauli_sum(st, 1, one.offsets.data(), one.qubits.data(), nullptr, nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        EXPECT(qsv_expect_pauli_sum(st, -1, one.offsets.data(), one.qubits.data(), one.letters.data(), nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        // ---- offsets: decreasing, negative start, a term of 65 letters ------------------------------------------------
        {
            const int down[3] = {0, 1, 0}, negative[2] = {-1, 0};
            const int qs[2] = {0, 0};
            EXPECT(qsv_expect_pauli_sum(st, 2, down, qs, "ZZ", nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
            EXPECT(qsv_expect_pauli_sum(st, 1, negative, qs, "ZZ", nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
            const int wide[2] = {0, 65};
            std::vector<int> many(65);
            for (int j = 0; j < 65; ++j) many[j] = j;
            const std::string zs(65, 'Z');
            EXPECT(qsv_expect_pauli_sum(st, 1, wide, many.data(), zs.data(), nullptr, nullptr, &re, &im, nullptr) == QSV_EINVAL);
        }
        // ---- a bad term anywhere in the list stops the call before its first launch --------------------------------------
        for (int bad = 0; bad < 4; ++bad) {
            Terms t;
            t.add("Z", {0});
            t.add("x", {n - 1});
            if (bad == 0) t.add("Q", {0});                             // a bad letter
            if (bad == 1) t.add("ZZ", {0, 0});                         // a repeated qubit
            if (bad == 2) t.add("Z", {n});                             // out of range
            if (bad == 3) t.add("Z", {-1});
            before = qsv_stub_launches;
            EXPECT(run(st, t, nullptr, nullptr, &re, &im, &passes) == QSV_EINVAL);
            EXPECT(qsv_stub_launches == before);
        }
        // ---- valid lists: identity and empty terms, every letter in both cases, every qubit as the pivot, groups of 1 .. 40 -
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
                    t.add("Zx", {q, q + 1});
                }
            }
            std::vector<double> coeffs(2 * t.count()), values(t.count(), 5.0);
            for (size_t j = 0; j < coeffs.size(); ++j) coeffs[j] = 0.25 * static_cast<double>(j % 7) - 0.5;
            before = qsv_stub_launches;
            EXPECT(run(st, t, coeffs.data(), values.data(), &re, &im, &passes) == QSV_OK);
            EXPECT(passes >= 1 && qsv_stub_launches - before == passes);
            EXPECT(re == 0.0 && im == 0.0);
            for (double v : values) EXPECT(v == 0.0);
            EXPECT(run(st, t, nullptr, nullptr, &re, &im, nullptr) == QSV_OK);
        }
        for (int count : {1, 7, 8, 9, 16, 17, 40}) {
            Terms t;
            for (int j = 0; j < count; ++j) {
                if (n >= 2) t.add(j % 2 ? "XZ" : "XI", {0, 1 + j % (n - 1)});
                else t.add(j % 2 ? "X" : "x", {0});
            }
            before = qsv_stub_launches;
            EXPECT(run(st, t, nullptr, nullptr, &re, &im, &passes) == QSV_OK);
            EXPECT(passes == static_cast<uint64_t>((count + 7) / 8) && qsv_stub_launches - before == passes);
        }
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- a view on caller-owned memory, and a mode register (refused) ------------------------------------------------------
    {
        std::vector<double> mem(2 * 64, 0.0);
        qsv_state *st = nullptr;
        EXPECT(qsv_create_view(6, 0, mem.data(), 64, nullptr, &st) == QSV_OK);
        Terms t;
        t.add("XY", {5, 0});
        t.add("ZZ", {2, 3});
        double re = 1.0, im = 1.0, values[2] = {1.0, 1.0};
        uint64_t passes = 0;
        EXPECT(run(st, t, nullptr, values, &re, &im, &passes) == QSV_OK && passes == 2);
        EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_create_qudit(3, 3, 0, &st) == QSV_OK);
        EXPECT(run(st, t, nullptr, values, &re, &im, &passes) == QSV_ESTATE);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("Pauli-sum");
}

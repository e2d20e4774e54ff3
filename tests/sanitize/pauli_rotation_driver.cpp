// TEST INFRASTRUCTURE: drives the host side of qsv_apply_pauli_rotation / qsv_apply_pauli_rotations -- every validation
// branch, the parsing of the flattened term list, the greedy planner and the launch of every pass -- under ASan + UBSan
// against hip_stub.cpp (device memory is zeroed host memory and kernels do not run).  The number of launches of every
// valid call is compared with a model of the greedy rule written here on the letters themselves.
// Walks: null pointers, a negative count, decreasing offsets, a term of 65 letters, repeated and out-of-range qubits, a bad
// letter, a mode register -- each refused before any launch and with the deferred queue left alone -- and then valid lists
// on registers of 1 to 18 qubits and on a view.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "driver_common.h"

struct Terms {
    std::vector<int> offsets = {0}, qubits;
    std::string letters;
    std::vector<double> thetas;
    void add(const std::string &paulis, const std::vector<int> &qs) {
        letters += paulis;
        qubits.insert(qubits.end(), qs.begin(), qs.end());
        offsets.push_back(static_cast<int>(qubits.size()));
        thetas.push_back(0.125 * static_cast<double>(thetas.size() % 9) - 0.5);
    }
    int count() const { return static_cast<int>(thetas.size()); }
    // the greedy rule on the flipped-qubit sets: a term joins the open pass if the pass holds fewer than 8 terms and the
    // term flips nothing, the pass flips nothing yet, or both flip the same qubits
    uint64_t model_passes() const {
        uint64_t passes = 0, open_flips = 0;
        int held = 0;
        for (int t = 0; t < count(); ++t) {
            uint64_t flips = 0;
            for (int j = offsets[t]; j < offsets[t + 1]; ++j)
                if (std::strchr("XxYy", letters[j])) flips |= 1ull << qubits[j];
            if (passes == 0 || held == 8 || !(flips == 0 || open_flips == 0 || flips == open_flips)) {
                ++passes;
                held = 0;
                open_flips = 0;
            }
            if (open_flips == 0) open_flips = flips;
            ++held;
        }
        return passes;
    }
};

static int run(qsv_state *st, const Terms &t, uint64_t *passes) {
    return qsv_apply_pauli_rotations(st, t.count(), t.offsets.data(), t.qubits.data(), t.letters.data(), t.thetas.data(), passes);
}

static void expect_valid(qsv_state *st, const Terms &t) {
    uint64_t passes = 99;
    const unsigned long before = qsv_stub_launches;
    EXPECT(run(st, t, &passes) == QSV_OK);
    EXPECT(passes == t.model_passes() && qsv_stub_launches - before == passes);
    EXPECT(run(st, t, nullptr) == QSV_OK);
}

int main() {
    for (int n : {1, 2, 3, 6, 7, 13, 14, 18}) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        uint64_t passes = 99;
        // ---- the empty list: nothing happens, no pointer needed ---------------------------------------------------------
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_pauli_rotations(st, 0, nullptr, nullptr, nullptr, nullptr, &passes) == QSV_OK);
        EXPECT(passes == 0 && qsv_stub_launches == before);
        // ---- null pointers, negative counts -------------------------------------------------------------------------------
        Terms one;
        one.add("Z", {0});
        before = qsv_stub_launches;
        EXPECT(run(nullptr, one, nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotations(st, 1, nullptr, one.qubits.data(), one.letters.data(), one.thetas.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotations(st, 1, one.offsets.data(), nullptr, one.letters.data(), one.thetas.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotations(st, 1, one.offsets.data(), one.qubits.data(), nullptr, one.thetas.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotations(st, 1, one.offsets.data(), one.qubits.data(), one.letters.data(), nullptr, nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotations(st, -1, one.offsets.data(), one.qubits.data(), one.letters.data(), one.thetas.data(), nullptr) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotation(nullptr, 1, one.qubits.data(), "Z", 0.3) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotation(st, 1, nullptr, "Z", 0.3) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotation(st, 1, one.qubits.data(), nullptr, 0.3) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotation(st, -1, one.qubits.data(), "Z", 0.3) == QSV_EINVAL);
        // ---- offsets: decreasing, negative start, a term of 65 letters ----------------------------------------------------
        {
            const int down[3] = {0, 1, 0}, negative[2] = {-1, 0};
            const int qs[2] = {0, 0};
            const double thetas[2] = {0.1, 0.2};
            EXPECT(qsv_apply_pauli_rotations(st, 2, down, qs, "ZZ", thetas, nullptr) == QSV_EINVAL);
            EXPECT(qsv_apply_pauli_rotations(st, 1, negative, qs, "ZZ", thetas, nullptr) == QSV_EINVAL);
            const int wide[2] = {0, 65};
            std::vector<int> many(65);
            for (int j = 0; j < 65; ++j) many[j] = j;
            const std::string zs(65, 'Z');
            EXPECT(qsv_apply_pauli_rotations(st, 1, wide, many.data(), zs.data(), thetas, nullptr) == QSV_EINVAL);
            EXPECT(qsv_apply_pauli_rotation(st, 65, many.data(), zs.data(), 0.1) == QSV_EINVAL);
        }
        // ---- a bad term anywhere in the list stops the call before its first launch ------------------------------------------
        for (int bad = 0; bad < 4; ++bad) {
            Terms t;
            t.add("Z", {0});
            t.add("x", {n - 1});
            if (bad == 0) t.add("Q", {0});                             // a bad letter
            if (bad == 1) t.add("ZZ", {0, 0});                         // a repeated qubit
            if (bad == 2) t.add("Z", {n});                             // out of range
            if (bad == 3) t.add("Z", {-1});
            EXPECT(run(st, t, &passes) == QSV_EINVAL);
            const int q = bad == 2 ? n : bad == 3 ? -1 : 0;
            EXPECT(qsv_apply_pauli_rotation(st, 1, &q, bad == 0 ? "Q" : "Z", 0.2) == (bad == 1 ? QSV_OK : QSV_EINVAL));
        }
        EXPECT(qsv_stub_launches == before + 1);                       // the one valid single call above (bad == 1: "Z" on qubit 0)
        // ---- single calls: every letter in both cases, the identity and k = 0: one launch each ----------------------------------
        before = qsv_stub_launches;
        {
            const int q0 = 0, qlast = n - 1;
            for (const char *letter : {"I", "i", "X", "x", "Y", "y", "Z", "z"}) {
                EXPECT(qsv_apply_pauli_rotation(st, 1, &q0, letter, 0.7) == QSV_OK);
                EXPECT(qsv_apply_pauli_rotation(st, 1, &qlast, letter, -0.7) == QSV_OK);
            }
            EXPECT(qsv_apply_pauli_rotation(st, 0, nullptr, nullptr, 1.0) == QSV_OK);
            EXPECT(qsv_stub_launches - before == 17);
            std::vector<int> all(n);
            for (int j = 0; j < n; ++j) all[j] = j;
            for (char letter : {'I', 'X', 'Y', 'Z'}) EXPECT(qsv_apply_pauli_rotation(st, n, all.data(), std::string(n, letter).data(), 0.3) == QSV_OK);
        }
        // ---- valid lists: identity and empty terms, every qubit as the pivot, diagonal terms riding along ---------------------------
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
            expect_valid(st, t);
        }
        for (int count : {1, 7, 8, 9, 16, 17, 25, 40}) {
            Terms shared, diagonal, alternating;
            for (int j = 0; j < count; ++j) {
                if (n >= 2) shared.add(j % 2 ? "XZ" : "XI", {0, 1 + j % (n - 1)});
                else shared.add(j % 2 ? "X" : "y", {0});
                diagonal.add(j % 3 ? "Z" : "I", {j % n});
                alternating.add(j % 2 ? "X" : "Y", {j % 2 ? 0 : n - 1});
            }
            expect_valid(st, shared);
            expect_valid(st, diagonal);
            expect_valid(st, alternating);
            EXPECT(shared.model_passes() == static_cast<uint64_t>((count + 7) / 8));
            EXPECT(diagonal.model_passes() == static_cast<uint64_t>((count + 7) / 8));
            if (n >= 2) EXPECT(alternating.model_passes() == static_cast<uint64_t>(count));
        }
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- a deferring register: a refused call leaves the queue alone, a valid one flushes it first --------------------------
    {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(13, 0, &st) == QSV_OK);
        EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        uint64_t queued = 0, launched = 0, queued_after = 0, launched_after = 0;
        EXPECT(qsv_apply_1q(st, 3, h) == QSV_OK);
        EXPECT(qsv_defer_stats(st, &queued, &launched) == QSV_OK);
        unsigned long before = qsv_stub_launches;
        const int bad = 13, good = 12;
        EXPECT(qsv_apply_pauli_rotation(st, 1, &bad, "X", 0.4) == QSV_EINVAL);
        EXPECT(qsv_apply_pauli_rotation(st, 1, &good, "Q", 0.4) == QSV_EINVAL);
        EXPECT(qsv_defer_stats(st, &queued_after, &launched_after) == QSV_OK);
        EXPECT(queued == 1 && queued_after == 1 && launched_after == launched && qsv_stub_launches == before);
        EXPECT(qsv_apply_pauli_rotation(st, 1, &good, "X", 0.4) == QSV_OK);
        EXPECT(qsv_defer_stats(st, &queued_after, &launched_after) == QSV_OK);
        EXPECT(launched_after == launched + 1 && queued_after == 1);   // the queued gate went out; the rotation was never queued
        EXPECT(qsv_stub_launches == before + 2);
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
        t.add("yx", {0, 5});
        t.add("XY", {4, 0});
        uint64_t passes = 0;
        EXPECT(run(st, t, &passes) == QSV_OK && passes == 2);
        expect_valid(st, t);
        EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_create_qudit(3, 3, 0, &st) == QSV_OK);
        const int q = 0;
        EXPECT(run(st, t, &passes) == QSV_ESTATE);
        EXPECT(qsv_apply_pauli_rotation(st, 1, &q, "Z", 0.1) == QSV_ESTATE);
        EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("Pauli-rotation");
}

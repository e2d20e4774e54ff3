// TEST INFRASTRUCTURE: drives the host side of the diagonal-operator entry points (qsv_diag_*, qsv_apply_diag_phase / _mul,
// qsv_expect_diag, qsv_diag_transition, qsv_diag_phase_adjoint) -- every refusal, the term packer, the windows of upload and
// download, the scratch slices and the launch of every pass -- under ASan + UBSan against hip_stub.cpp (device memory is
// zeroed host memory and kernels do not run).  Launches are counted: one per build whatever the number of terms, one per
// register x diagonal pass.
// Walks: null handles, bad sizes and devices, options other than the grid cap, windows of upload and download out of
// bounds, X / Y letters, qubits out of range or repeated, 65 letters, registers and diagonals of different sizes, a
// destination that is too small or meets its source, mode registers -- each refused before any launch and with every
// deferred queue left alone -- and then valid calls for 0 to 18 qubits with 0, 1, 2, 63, 64, 65 and 200 terms, windows at
// both ends and `accumulate`.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "driver_common.h"

// exactly as many entries as the call may read: a read past the caller's arrays is an ASan report
struct Terms {
    std::vector<int> offsets{0}, qubits;
    std::vector<char> letters;
    std::vector<double> coeffs;
    void add(const std::string &l, const std::vector<int> &q, double c) {
        letters.insert(letters.end(), l.begin(), l.end());
        qubits.insert(qubits.end(), q.begin(), q.end());
        offsets.push_back(static_cast<int>(qubits.size()));
        coeffs.push_back(c);
    }
    int count() const { return static_cast<int>(coeffs.size()); }
    const int *q() const { return qubits.empty() ? nullptr : qubits.data(); }
    const char *l() const { return letters.empty() ? nullptr : letters.data(); }
};

static Terms some_terms(int n, int count) {
    Terms t;
    unsigned state = 12345u + 77u * n + count;
    for (int k = 0; k < count; ++k) {
        state = state * 1664525u + 1013904223u;
        if (n == 0 || k % 7 == 2) {
            t.add("", {}, 0.5 * k);                              // the identity term
        } else if (n == 1 || k % 3 == 0) {
            t.add("Z", {static_cast<int>((state >> 8) % n)}, 1.0 - 0.01 * k);
        } else {
            const int a = static_cast<int>((state >> 8) % n), b = (a + 1 + static_cast<int>((state >> 20) % (n - 1))) % n;
            t.add(k % 2 ? "ZZ" : "zI", {a, b}, -0.25 * k);
        }
    }
    return t;
}

static int set_terms(qsv_diag *d, const Terms &t, int accumulate, uint64_t *passes) {
    return qsv_diag_set_pauli_sum(d, t.count(), t.offsets.data(), t.q(), t.l(), t.coeffs.data(), accumulate, passes);
}

static void diag_refusals(qsv_diag *d, int n) {
    const unsigned long before = qsv_stub_launches;
    const uint64_t size = 1ull << n;
    std::vector<double> buf(size + 1, 1.0);
    int qubits = -1;
    uint64_t passes = 99;
    EXPECT(qsv_diag_num_qubits(nullptr, &qubits) == QSV_EINVAL && qsv_diag_num_qubits(d, nullptr) == QSV_EINVAL);
    EXPECT(qsv_diag_num_qubits(d, &qubits) == QSV_OK && qubits == n);
    EXPECT(qsv_diag_set_stream(nullptr, nullptr) == QSV_EINVAL && qsv_diag_set_stream(d, nullptr) == QSV_OK);
    EXPECT(qsv_diag_set_option(nullptr, QSV_OPT_GRID_CAP, 2) == QSV_EINVAL);
    EXPECT(qsv_diag_set_option(d, QSV_OPT_NONTEMPORAL, 0) == QSV_EINVAL && qsv_diag_set_option(d, QSV_OPT_DEFER, 0) == QSV_EINVAL);
    EXPECT(qsv_diag_set_option(d, QSV_OPT_GRID_CAP, -1) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(nullptr, buf.data(), 0, 1) == QSV_EINVAL && qsv_diag_download(nullptr, buf.data(), 0, 1) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, nullptr, 0, 1) == QSV_EINVAL && qsv_diag_download(d, nullptr, 0, 1) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, buf.data(), 0, size + 1) == QSV_EINVAL && qsv_diag_download(d, buf.data(), 0, size + 1) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, buf.data(), size + 1, 0) == QSV_EINVAL && qsv_diag_download(d, buf.data(), size + 1, 0) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, buf.data(), size, 1) == QSV_EINVAL && qsv_diag_download(d, buf.data(), 1, size) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, buf.data(), 1, ~0ull) == QSV_EINVAL && qsv_diag_download(d, buf.data(), 1, ~0ull) == QSV_EINVAL);
    EXPECT(qsv_diag_upload(d, nullptr, size, 0) == QSV_OK && qsv_diag_download(d, nullptr, 0, 0) == QSV_OK);      // empty windows
    EXPECT(qsv_diag_extrema(nullptr, nullptr, nullptr, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_diag_last_kernel(nullptr, nullptr, 0) == QSV_EINVAL);
    // the term list: everything before any launch
    const Terms good = some_terms(n, 5);
    EXPECT(set_terms(nullptr, good, 0, &passes) == QSV_EINVAL);
    EXPECT(qsv_diag_set_pauli_sum(d, -1, good.offsets.data(), good.q(), good.l(), good.coeffs.data(), 0, &passes) == QSV_EINVAL);
    EXPECT(qsv_diag_set_pauli_sum(d, 2, nullptr, good.q(), good.l(), good.coeffs.data(), 0, &passes) == QSV_EINVAL);
    if (n >= 1) {
        for (const char *letter : {"X", "Y", "x", "y", "Q"}) {
            Terms bad = some_terms(n, 3);
            bad.add(letter, {0}, 1.0);
            EXPECT(set_terms(d, bad, 0, &passes) == QSV_EINVAL);
        }
        Terms range = some_terms(n, 3), negative = some_terms(n, 3), many = some_terms(n, 2);
        range.add("Z", {n}, 1.0);
        negative.add("Z", {-1}, 1.0);
        EXPECT(set_terms(d, range, 0, &passes) == QSV_EINVAL && set_terms(d, negative, 1, &passes) == QSV_EINVAL);
        std::vector<int> q65(65);
        for (int k = 0; k < 65; ++k) q65[k] = k % n;
        many.add(std::string(65, 'I'), q65, 1.0);
        EXPECT(set_terms(d, many, 0, &passes) == QSV_EINVAL);
    }
    if (n >= 2) {
        Terms repeat = some_terms(n, 3);
        repeat.add("ZZ", {1, 1}, 1.0);
        EXPECT(set_terms(d, repeat, 0, &passes) == QSV_EINVAL);
    }
    EXPECT(qsv_stub_launches == before);
}

static void diag_valid(qsv_diag *d, int n) {
    const uint64_t size = 1ull << n;
    // windows of upload and download at both ends
    std::vector<double> all(size), back(size, -1.0);
    for (uint64_t i = 0; i < size; ++i) all[i] = 0.5 * static_cast<double>(i) - 3.0;
    EXPECT(qsv_diag_upload(d, all.data(), 0, size) == QSV_OK);
    EXPECT(qsv_diag_download(d, back.data(), 0, size) == QSV_OK && back == all);
    const uint64_t half = size / 2;
    std::vector<double> low(half + 1, 9.0), high(size - half + 1, 9.0);
    EXPECT(qsv_diag_download(d, low.data(), 0, half) == QSV_OK && low[half] == 9.0 && (half == 0 || low[half - 1] == all[half - 1]));
    EXPECT(qsv_diag_download(d, high.data(), half, size - half) == QSV_OK && high[size - half] == 9.0 && high[0] == all[half]);
    const double one = 123.0;
    double got = 0.0;
    EXPECT(qsv_diag_upload(d, &one, size - 1, 1) == QSV_OK && qsv_diag_download(d, &got, size - 1, 1) == QSV_OK && got == 123.0);
    EXPECT(qsv_diag_upload(d, &one, 0, 1) == QSV_OK && qsv_diag_download(d, &got, 0, 1) == QSV_OK && got == 123.0);
    // one launch per build, whatever the number of terms
    for (int cap : {0, 2}) {
        EXPECT(qsv_diag_set_option(d, QSV_OPT_GRID_CAP, cap) == QSV_OK);
        for (int count : {0, 1, 2, 63, 64, 65, 200}) {
            const Terms t = some_terms(n, count);
            for (int accumulate = 0; accumulate < 2; ++accumulate) {
                uint64_t passes = 99;
                const unsigned long before = qsv_stub_launches;
                EXPECT(set_terms(d, t, accumulate, &passes) == QSV_OK);
                const uint64_t want = count == 0 && accumulate ? 0 : 1;
                EXPECT(passes == want && qsv_stub_launches - before == want);
                EXPECT(set_terms(d, t, accumulate, nullptr) == QSV_OK);
            }
            // no coefficients: all 1
            EXPECT(qsv_diag_set_pauli_sum(d, t.count(), t.offsets.data(), t.q(), t.l(), nullptr, 0, nullptr) == QSV_OK);
        }
        char name[64] = "";
        EXPECT(qsv_diag_last_kernel(d, name, sizeof(name)) == QSV_OK && std::strcmp(name, "k_diag_build<false>") == 0);
        double mn = 7.0, mx = 7.0;
        uint64_t amn = 7, amx = 7;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_diag_extrema(d, &mn, &amn, &mx, &amx) == QSV_OK && qsv_stub_launches == before + 1);
        EXPECT(qsv_diag_extrema(d, nullptr, nullptr, nullptr, nullptr) == QSV_OK && qsv_diag_extrema(d, &mn, nullptr, nullptr, &amx) == QSV_OK);
        EXPECT(qsv_diag_last_kernel(d, name, sizeof(name)) == QSV_OK && std::strcmp(name, "k_diag_extrema") == 0);
    }
    EXPECT(qsv_diag_set_option(d, QSV_OPT_GRID_CAP, 0) == QSV_OK);
}

// every refusal of the register x diagonal passes on registers a, b and a diagonal d of one size; nothing may be launched
static void pass_refusals(qsv_state *a, qsv_state *b, qsv_diag *d) {
    double out[4] = {0, 0, 0, 0}, re = 0.0, im = 0.0;
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_apply_diag_phase(nullptr, d, 0.3) == QSV_EINVAL && qsv_apply_diag_phase(a, nullptr, 0.3) == QSV_EINVAL);
    EXPECT(qsv_apply_diag_mul(nullptr, a, d, 1, 0, 0) == QSV_EINVAL && qsv_apply_diag_mul(b, nullptr, d, 1, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_apply_diag_mul(b, a, nullptr, 1, 0, 0) == QSV_EINVAL);
    EXPECT(qsv_apply_diag_mul(a, a, d, 1, 0, 1) == QSV_EINVAL);                    // in place only when not accumulating
    EXPECT(qsv_expect_diag(nullptr, d, nullptr, out) == QSV_EINVAL && qsv_expect_diag(a, nullptr, nullptr, out) == QSV_EINVAL);
    EXPECT(qsv_expect_diag(a, d, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_diag_transition(nullptr, a, d, &re, &im) == QSV_EINVAL && qsv_diag_transition(a, nullptr, d, &re, &im) == QSV_EINVAL);
    EXPECT(qsv_diag_transition(a, b, nullptr, &re, &im) == QSV_EINVAL && qsv_diag_transition(a, b, d, nullptr, &im) == QSV_EINVAL);
    EXPECT(qsv_diag_transition(a, b, d, &re, nullptr) == QSV_EINVAL);
    EXPECT(qsv_diag_phase_adjoint(nullptr, b, d, 0.1, &re, &im) == QSV_EINVAL && qsv_diag_phase_adjoint(a, nullptr, d, 0.1, &re, &im) == QSV_EINVAL);
    EXPECT(qsv_diag_phase_adjoint(a, b, nullptr, 0.1, &re, &im) == QSV_EINVAL && qsv_diag_phase_adjoint(a, b, d, 0.1, nullptr, &im) == QSV_EINVAL);
    EXPECT(qsv_diag_phase_adjoint(a, a, d, 0.1, &re, &im) == QSV_EINVAL);          // two registers
    EXPECT(qsv_stub_launches == before);
}

static void pass_valid(qsv_state *a, qsv_state *b, qsv_diag *d) {
    double out[5] = {7, 7, 7, 7, 7}, re = 7.0, im = 7.0;
    const double threshold = 0.5;
    char name[96] = "";
    for (int cap : {0, 2}) {
        EXPECT(qsv_set_option(a, QSV_OPT_GRID_CAP, cap) == QSV_OK && qsv_set_option(b, QSV_OPT_GRID_CAP, cap) == QSV_OK);
        for (int nt = 0; nt < 2; ++nt) {
            EXPECT(qsv_set_option(a, QSV_OPT_NONTEMPORAL, nt) == QSV_OK && qsv_set_option(b, QSV_OPT_NONTEMPORAL, nt) == QSV_OK);
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_apply_diag_phase(a, d, 0.3) == QSV_OK);
            EXPECT(qsv_last_kernel(a, name, sizeof(name)) == QSV_OK && std::strcmp(name, nt ? "k_diag_phase<true>" : "k_diag_phase<false>") == 0);
            EXPECT(qsv_apply_diag_mul(b, a, d, 0.5, -0.25, 0) == QSV_OK && qsv_apply_diag_mul(b, a, d, 0.5, -0.25, 1) == QSV_OK);
            EXPECT(qsv_apply_diag_mul(a, a, d, 2.0, 0.0, 0) == QSV_OK);                // D psi in place
            EXPECT(qsv_expect_diag(a, d, nullptr, out) == QSV_OK && out[4] == 7.0);    // four values, not five
            EXPECT(qsv_expect_diag(a, d, &threshold, out) == QSV_OK && out[0] == 0.0 && out[3] == 0.0 && out[4] == 7.0);
            EXPECT(qsv_diag_transition(a, b, d, &re, &im) == QSV_OK && re == 0.0 && im == 0.0);
            EXPECT(qsv_diag_transition(a, a, d, &re, &im) == QSV_OK);                  // the same register twice
            EXPECT(qsv_diag_phase_adjoint(a, b, d, -0.3, &re, &im) == QSV_OK);
            EXPECT(qsv_last_kernel(a, name, sizeof(name)) == QSV_OK &&
                   std::strcmp(name, nt ? "k_diag_phase_adjoint<true>" : "k_diag_phase_adjoint<false>") == 0);
            EXPECT(qsv_stub_launches - before == 9);                                   // one launch per call
        }
    }
    EXPECT(qsv_set_option(a, QSV_OPT_GRID_CAP, 0) == QSV_OK && qsv_set_option(b, QSV_OPT_GRID_CAP, 0) == QSV_OK);
}

int main() {
    {
        qsv_diag *d = nullptr;
        EXPECT(qsv_diag_create(3, 0, nullptr) == QSV_EINVAL);
        EXPECT(qsv_diag_create(-1, 0, &d) == QSV_EINVAL && d == nullptr);
        EXPECT(qsv_diag_create(41, 0, &d) == QSV_EINVAL && d == nullptr);
        EXPECT(qsv_diag_create(3, 1, &d) == QSV_EINVAL && d == nullptr);               // the stand-in runtime has one device
        EXPECT(qsv_diag_create(3, -1, &d) == QSV_EINVAL && d == nullptr);
        EXPECT(qsv_diag_destroy(nullptr) == QSV_OK);
    }
    for (int n = 0; n <= 18; ++n) {
        qsv_diag *d = nullptr;
        qsv_state *a = nullptr, *b = nullptr;
        EXPECT(qsv_diag_create(n, 0, &d) == QSV_OK && d != nullptr);
        double first = 1.0, last = 1.0;
        EXPECT(qsv_diag_download(d, &first, 0, 1) == QSV_OK && qsv_diag_download(d, &last, (1ull << n) - 1, 1) == QSV_OK);
        EXPECT(first == 0.0 && last == 0.0);                                           // zero-filled
        diag_refusals(d, n);
        diag_valid(d, n);
        EXPECT(qsv_create(n, 0, &a) == QSV_OK && qsv_create(n, 0, &b) == QSV_OK);
        pass_refusals(a, b, d);
        pass_valid(a, b, d);
        // sizes: register and diagonal of one size; dst takes src's size if it has the room
        if (n >= 1) {
            qsv_state *small = nullptr;
            qsv_diag *small_d = nullptr;
            double out[4], re, im;
            int qubits = 0;
            EXPECT(qsv_create(n - 1, 0, &small) == QSV_OK && qsv_diag_create(n - 1, 0, &small_d) == QSV_OK);
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_apply_diag_phase(small, d, 0.1) == QSV_EINVAL && qsv_apply_diag_phase(a, small_d, 0.1) == QSV_EINVAL);
            EXPECT(qsv_expect_diag(small, d, nullptr, out) == QSV_EINVAL && qsv_expect_diag(a, small_d, nullptr, out) == QSV_EINVAL);
            EXPECT(qsv_diag_transition(a, small, d, &re, &im) == QSV_EINVAL && qsv_diag_transition(small, a, d, &re, &im) == QSV_EINVAL);
            EXPECT(qsv_diag_transition(a, b, small_d, &re, &im) == QSV_EINVAL);
            EXPECT(qsv_diag_phase_adjoint(a, small, d, 0.1, &re, &im) == QSV_EINVAL && qsv_diag_phase_adjoint(small, a, d, 0.1, &re, &im) == QSV_EINVAL);
            EXPECT(qsv_diag_phase_adjoint(a, b, small_d, 0.1, &re, &im) == QSV_EINVAL);
            EXPECT(qsv_apply_diag_mul(small, a, d, 1, 0, 0) == QSV_ENOMEM);            // no room
            EXPECT(qsv_apply_diag_mul(b, a, small_d, 1, 0, 0) == QSV_EINVAL);
            EXPECT(qsv_apply_diag_mul(b, small, small_d, 1, 0, 1) == QSV_EINVAL);      // accumulating needs the size already
            EXPECT(qsv_stub_launches == before);
            EXPECT(qsv_apply_diag_mul(b, small, small_d, 1, 0, 0) == QSV_OK);          // b shrinks ...
            EXPECT(qsv_num_qubits(b, &qubits) == QSV_OK && qubits == n - 1);
            EXPECT(qsv_apply_diag_mul(b, a, d, 1, 0, 0) == QSV_OK);                    // ... and grows back inside its allocation
            EXPECT(qsv_num_qubits(b, &qubits) == QSV_OK && qubits == n);
            EXPECT(qsv_destroy(small) == QSV_OK && qsv_diag_destroy(small_d) == QSV_OK);
        }
        EXPECT(qsv_destroy(a) == QSV_OK && qsv_destroy(b) == QSV_OK && qsv_diag_destroy(d) == QSV_OK);
    }
    // ---- deferring registers: a refused call leaves every queue alone, a valid one flushes every register first ------------
    for (int call = 0; call < 5; ++call) {
        qsv_state *regs[2] = {nullptr, nullptr};
        qsv_diag *d = nullptr, *wrong = nullptr;
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        uint64_t queued[2], launched[2], after = 0, now = 0;
        double out[4], re, im;
        EXPECT(qsv_diag_create(13, 0, &d) == QSV_OK && qsv_diag_create(12, 0, &wrong) == QSV_OK);
        for (int k = 0; k < 2; ++k) {
            EXPECT(qsv_create(13, 0, &regs[k]) == QSV_OK);
            EXPECT(qsv_set_option(regs[k], QSV_OPT_DEFER, 2) == QSV_OK);
            EXPECT(qsv_apply_1q(regs[k], 3 + k, h) == QSV_OK);
            EXPECT(qsv_defer_stats(regs[k], &queued[k], &launched[k]) == QSV_OK && queued[k] == 1);
        }
        auto make = [&](qsv_diag *dd) {
            switch (call) {
                case 0: return qsv_apply_diag_phase(regs[0], dd, 0.3);
                case 1: return qsv_apply_diag_mul(regs[0], regs[1], dd, 1.0, 0.0, 0);
                case 2: return qsv_expect_diag(regs[0], dd, nullptr, out);
                case 3: return qsv_diag_transition(regs[0], regs[1], dd, &re, &im);
                default: return qsv_diag_phase_adjoint(regs[0], regs[1], dd, 0.3, &re, &im);
            }
        };
        const int used = call == 0 || call == 2 ? 1 : 2;
        const unsigned long before = qsv_stub_launches;
        EXPECT(make(wrong) == QSV_EINVAL);
        for (int k = 0; k < 2; ++k) EXPECT(qsv_defer_stats(regs[k], &after, &now) == QSV_OK && after == 1 && now == launched[k]);
        EXPECT(qsv_stub_launches == before);
        EXPECT(make(d) == QSV_OK);
        for (int k = 0; k < used; ++k) EXPECT(qsv_defer_stats(regs[k], &after, &now) == QSV_OK && after == 1 && now == launched[k] + 1);
        EXPECT(qsv_stub_launches == before + used + 1);            // the queued gates and the call's one pass
        for (qsv_state *st : regs) EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_diag_destroy(d) == QSV_OK && qsv_diag_destroy(wrong) == QSV_OK);
    }
    // ---- views on caller-owned memory and mode registers ---------------------------------------------------------------------
    {
        std::vector<double> mem(2 * 160, 0.0);
        qsv_state *low = nullptr, *mid = nullptr, *high = nullptr, *owned = nullptr, *modes = nullptr;
        qsv_diag *d = nullptr;
        double out[4], re, im;
        EXPECT(qsv_create_view(6, 0, mem.data(), 64, nullptr, &low) == QSV_OK);
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 32, 64, nullptr, &mid) == QSV_OK);       // amplitudes 32..95: meets both
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 64, 96, nullptr, &high) == QSV_OK);      // amplitudes 64..127
        EXPECT(qsv_create(6, 0, &owned) == QSV_OK && qsv_create_qudit(3, 3, 0, &modes) == QSV_OK && qsv_diag_create(6, 0, &d) == QSV_OK);
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_diag_mul(low, mid, d, 1, 0, 0) == QSV_EINVAL && qsv_apply_diag_mul(high, mid, d, 1, 0, 1) == QSV_EINVAL);
        EXPECT(qsv_diag_phase_adjoint(low, mid, d, 0.1, &re, &im) == QSV_EINVAL);
        EXPECT(qsv_apply_diag_phase(modes, d, 0.1) == QSV_ESTATE && qsv_expect_diag(modes, d, nullptr, out) == QSV_ESTATE);
        EXPECT(qsv_apply_diag_mul(modes, owned, d, 1, 0, 0) == QSV_ESTATE && qsv_apply_diag_mul(owned, modes, d, 1, 0, 0) == QSV_ESTATE);
        EXPECT(qsv_diag_transition(modes, owned, d, &re, &im) == QSV_ESTATE && qsv_diag_transition(owned, modes, d, &re, &im) == QSV_ESTATE);
        EXPECT(qsv_diag_phase_adjoint(modes, owned, d, 0.1, &re, &im) == QSV_ESTATE && qsv_diag_phase_adjoint(owned, modes, d, 0.1, &re, &im) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_apply_diag_mul(low, high, d, 1, 0, 0) == QSV_OK && qsv_apply_diag_mul(low, high, d, 1, 0, 1) == QSV_OK);
        EXPECT(qsv_diag_transition(low, mid, d, &re, &im) == QSV_OK);                          // read-only: any windows
        pass_valid(low, high, d);
        pass_valid(owned, mid, d);
        for (qsv_state *st : {low, mid, high, owned, modes}) EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_diag_destroy(d) == QSV_OK);
    }
    return finish("diagonal");
}

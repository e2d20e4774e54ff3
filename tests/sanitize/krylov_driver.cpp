// TEST INFRASTRUCTURE: drives the host side of qsv_lincomb and qsv_inner_many -- every refusal, the split into passes,
// the argument builders, the slices of the scratch buffer and the launch of every pass -- under ASan + UBSan against
// hip_stub.cpp (device memory is zeroed host memory and kernels do not run).  The number of launches of every valid call
// is compared with ceil(operands / 8).
// Walks: null handles and arrays, a null entry inside an array, negative counts, the destination among the sources, views
// whose windows meet the destination's, registers of different sizes, a destination that is too small, mode registers --
// each refused before any launch and with every deferred queue left alone -- and then valid calls with 0 to 40 operands on
// registers of 1 to 18 qubits and on views (repeated and overlapping sources, x_k = y), with and without beta and the norm.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "driver_common.h"

static uint64_t passes_of(int operands) { return static_cast<uint64_t>((operands + 7) / 8); }

// exactly `count` entries each: a read past the caller's arrays is an ASan report
struct Operands {
    std::vector<qsv_state *> regs;
    std::vector<double> coeffs;
    Operands(const std::vector<qsv_state *> &pool, int count) {
        for (int k = 0; k < count; ++k) {
            regs.push_back(pool[k % pool.size()]);          // sources may repeat
            coeffs.push_back(0.5 + k);
            coeffs.push_back(-0.25 * k);
        }
    }
    int count() const { return static_cast<int>(regs.size()); }
};

static void expect_valid(qsv_state *dst, const std::vector<qsv_state *> &pool) {
    for (int count : {0, 1, 2, 3, 5, 7, 8, 9, 16, 17, 40}) {
        const Operands ops(pool, count);
        for (int variant = 0; variant < 6; ++variant) {
            const double beta_re = variant % 3 == 1 ? 1.0 : 0.0, beta_im = variant % 3 == 2 ? -0.5 : 0.0;
            double norm2 = 7.0;
            uint64_t passes = 99;
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_lincomb(dst, beta_re, beta_im, count, count ? ops.regs.data() : nullptr, count ? ops.coeffs.data() : nullptr,
                               variant < 3 ? nullptr : &norm2, &passes) == QSV_OK);
            const uint64_t want = count ? passes_of(count) : 1;
            EXPECT(passes == want && qsv_stub_launches - before == want);
            EXPECT(variant < 3 ? norm2 == 7.0 : norm2 == 0.0);           // zeroed partials in, zero out
            EXPECT(qsv_lincomb(dst, beta_re, beta_im, count, count ? ops.regs.data() : nullptr, count ? ops.coeffs.data() : nullptr, nullptr, nullptr) == QSV_OK);
        }
        if (count == 0) continue;
        std::vector<double> values(2 * static_cast<size_t>(count) + 1, 7.0);
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_inner_many(dst, count, ops.regs.data(), values.data(), &passes) == QSV_OK);
        EXPECT(passes == passes_of(count) && qsv_stub_launches - before == passes);
        EXPECT(values[0] == 0.0 && values[2 * static_cast<size_t>(count) - 1] == 0.0 && values[2 * static_cast<size_t>(count)] == 7.0);   // no write past the end
        std::vector<qsv_state *> with_self = ops.regs;
        with_self[count / 2] = dst;                                      // x_k == y is allowed
        EXPECT(qsv_inner_many(dst, count, with_self.data(), values.data(), nullptr) == QSV_OK);
    }
}

// every refusal on (dst, a, b), all of one size; nothing may be launched
static void expect_refusals(qsv_state *dst, qsv_state *a, qsv_state *b) {
    qsv_state *two[2] = {a, b}, *with_null[2] = {a, nullptr}, *with_dst[2] = {a, dst};
    const double c[4] = {1.0, 0.0, 0.5, -0.5};
    double values[4] = {0, 0, 0, 0}, norm2 = 0.0;
    uint64_t passes = 99;
    const unsigned long before = qsv_stub_launches;
    EXPECT(qsv_lincomb(nullptr, 0.0, 0.0, 2, two, c, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_lincomb(dst, 0.0, 0.0, 2, nullptr, c, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_lincomb(dst, 0.0, 0.0, 2, two, nullptr, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_lincomb(dst, 0.0, 0.0, 2, with_null, c, &norm2, &passes) == QSV_EINVAL);
    EXPECT(qsv_lincomb(dst, 0.0, 0.0, -1, two, c, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_lincomb(nullptr, 1.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_lincomb(dst, 0.0, 0.0, 2, with_dst, c, nullptr, nullptr) == QSV_EINVAL);       // dst among the sources
    EXPECT(qsv_lincomb(dst, 1.0, 0.0, 2, with_dst, c, &norm2, nullptr) == QSV_EINVAL);
    EXPECT(qsv_inner_many(nullptr, 2, two, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_inner_many(dst, 2, nullptr, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_inner_many(dst, 2, two, nullptr, nullptr) == QSV_EINVAL);
    EXPECT(qsv_inner_many(dst, 2, with_null, values, &passes) == QSV_EINVAL);
    EXPECT(qsv_inner_many(dst, -1, two, values, nullptr) == QSV_EINVAL);
    EXPECT(qsv_stub_launches == before);
    // no operands: nothing to do, no pointer needed
    EXPECT(qsv_inner_many(dst, 0, nullptr, nullptr, &passes) == QSV_OK && passes == 0);
    EXPECT(qsv_stub_launches == before);
}

int main() {
    for (int n : {1, 2, 3, 6, 7, 13, 14, 18}) {
        qsv_state *dst = nullptr;
        std::vector<qsv_state *> pool(3, nullptr);
        EXPECT(qsv_create(n, 0, &dst) == QSV_OK);
        for (qsv_state *&st : pool) EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        expect_refusals(dst, pool[0], pool[1]);
        expect_valid(dst, pool);
        // ---- sizes: dst takes the sources' size with beta == 0 if it has the room; otherwise the sizes must agree ----------
        if (n >= 2) {
            qsv_state *small = nullptr;
            EXPECT(qsv_create(n - 1, 0, &small) == QSV_OK);
            qsv_state *big[1] = {pool[0]}, *mixed[2] = {pool[0], small}, *little[1] = {small};
            const double c[4] = {1.0, 0.0, 0.5, -0.5};
            double values[4];
            const unsigned long before = qsv_stub_launches;
            EXPECT(qsv_lincomb(small, 0.0, 0.0, 1, big, c, nullptr, nullptr) == QSV_ENOMEM);
            EXPECT(qsv_lincomb(dst, 0.0, 0.0, 2, mixed, c, nullptr, nullptr) == QSV_EINVAL);
            EXPECT(qsv_lincomb(dst, 1.0, 0.0, 1, little, c, nullptr, nullptr) == QSV_EINVAL);
            EXPECT(qsv_inner_many(dst, 2, mixed, values, nullptr) == QSV_EINVAL);
            EXPECT(qsv_inner_many(small, 1, big, values, nullptr) == QSV_EINVAL);
            EXPECT(qsv_stub_launches == before);
            int qubits = 0;
            EXPECT(qsv_lincomb(dst, 0.0, 0.0, 1, little, c, nullptr, nullptr) == QSV_OK);       // dst shrinks to small's size ...
            EXPECT(qsv_num_qubits(dst, &qubits) == QSV_OK && qubits == n - 1);
            EXPECT(qsv_lincomb(dst, 0.0, 0.0, 1, big, c, nullptr, nullptr) == QSV_OK);          // ... and grows back inside its allocation
            EXPECT(qsv_num_qubits(dst, &qubits) == QSV_OK && qubits == n);
            EXPECT(qsv_destroy(small) == QSV_OK);
        }
        EXPECT(qsv_destroy(dst) == QSV_OK);
        for (qsv_state *st : pool) EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- deferring registers: a refused call leaves every queue alone, a valid one flushes all of them first --------------------
    for (int call = 0; call < 2; ++call) {
        qsv_state *regs[3] = {nullptr, nullptr, nullptr};
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        uint64_t queued[3], launched[3], after = 0, now = 0;
        for (int k = 0; k < 3; ++k) {
            EXPECT(qsv_create(13, 0, &regs[k]) == QSV_OK);
            EXPECT(qsv_set_option(regs[k], QSV_OPT_DEFER, 2) == QSV_OK);
            EXPECT(qsv_apply_1q(regs[k], 3 + k, h) == QSV_OK);
            EXPECT(qsv_defer_stats(regs[k], &queued[k], &launched[k]) == QSV_OK && queued[k] == 1);
        }
        const unsigned long before = qsv_stub_launches;
        qsv_state *bad[2] = {regs[1], regs[0]}, *good[2] = {regs[1], regs[2]};
        const double c[4] = {1.0, 0.0, 0.5, -0.5};
        double values[4];
        EXPECT((call == 0 ? qsv_lincomb(regs[0], 1.0, 0.0, 2, bad, c, nullptr, nullptr) : qsv_inner_many(regs[0], 2, good, nullptr, nullptr)) == QSV_EINVAL);
        for (int k = 0; k < 3; ++k) EXPECT(qsv_defer_stats(regs[k], &after, &now) == QSV_OK && after == 1 && now == launched[k]);
        EXPECT(qsv_stub_launches == before);
        EXPECT((call == 0 ? qsv_lincomb(regs[0], 1.0, 0.0, 2, good, c, nullptr, nullptr) : qsv_inner_many(regs[0], 2, good, values, nullptr)) == QSV_OK);
        for (int k = 0; k < 3; ++k) EXPECT(qsv_defer_stats(regs[k], &after, &now) == QSV_OK && after == 1 && now == launched[k] + 1);
        EXPECT(qsv_stub_launches == before + 4);               // three queued gates and the call's one pass
        for (qsv_state *st : regs) EXPECT(qsv_destroy(st) == QSV_OK);
    }
    // ---- views on caller-owned memory: a destination that meets a source is refused; sources may overlap; modes are refused ------
    {
        std::vector<double> mem(2 * 160, 0.0);
        qsv_state *low = nullptr, *mid = nullptr, *high = nullptr, *owned = nullptr, *modes = nullptr;
        EXPECT(qsv_create_view(6, 0, mem.data(), 64, nullptr, &low) == QSV_OK);
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 32, 64, nullptr, &mid) == QSV_OK);       // amplitudes 32..95: meets both
        EXPECT(qsv_create_view(6, 0, mem.data() + 2 * 64, 96, nullptr, &high) == QSV_OK);      // amplitudes 64..127 (room for 96)
        EXPECT(qsv_create(6, 0, &owned) == QSV_OK);
        EXPECT(qsv_create_qudit(3, 3, 0, &modes) == QSV_OK);
        const double c[4] = {1.0, 0.0, 0.5, -0.5};
        double values[4], norm2 = 0.0;
        uint64_t passes = 0;
        const unsigned long before = qsv_stub_launches;
        qsv_state *s_mid[2] = {owned, mid}, *s_overlap[2] = {low, mid}, *s_modes[2] = {owned, modes}, *s_low[2] = {low, owned};
        EXPECT(qsv_lincomb(low, 0.0, 0.0, 2, s_mid, c, nullptr, nullptr) == QSV_EINVAL);
        EXPECT(qsv_lincomb(high, 1.0, 0.0, 2, s_mid, c, nullptr, nullptr) == QSV_EINVAL);
        EXPECT(qsv_lincomb(modes, 0.0, 0.0, 2, s_low, c, nullptr, nullptr) == QSV_ESTATE);
        EXPECT(qsv_lincomb(high, 0.0, 0.0, 2, s_modes, c, nullptr, nullptr) == QSV_ESTATE);
        EXPECT(qsv_inner_many(modes, 2, s_low, values, nullptr) == QSV_ESTATE);
        EXPECT(qsv_inner_many(low, 2, s_modes, values, nullptr) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_lincomb(owned, 0.5, 0.5, 2, s_overlap, c, &norm2, &passes) == QSV_OK && passes == 1);  // overlapping sources
        EXPECT(qsv_lincomb(low, 0.0, 0.0, 1, &high, c, nullptr, &passes) == QSV_OK && passes == 1);
        EXPECT(qsv_inner_many(mid, 2, s_overlap, values, &passes) == QSV_OK && passes == 1);               // read-only: any windows
        expect_valid(high, {low, owned});
        expect_valid(owned, {low, mid, high});
        for (qsv_state *st : {low, mid, high, owned, modes}) EXPECT(qsv_destroy(st) == QSV_OK);
    }
    return finish("Krylov");
}

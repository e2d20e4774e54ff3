// TEST INFRASTRUCTURE: drives the host side of qsv_arith_create / qsv_apply_arith -- every validation branch, both parameter
// sets of every kind, the launch shape and the spare-buffer adoption -- under ASan + UBSan against hip_stub.cpp (device memory
// is zeroed host memory and kernels do not run).  The number of launches of every valid call is compared with what
// csrc/qsv_arith_layout.h (included here as the library includes it) says: one, or none for a map that moves nothing.
// Walks: every refusal of create; null pointers, a mode register, a handle on another device, repeated and out-of-range
// qubits across target, source and controls, unknown flag bits -- each refused before any launch and with the deferred queue
// left alone -- then valid calls of every kind, forward and inverse, on plain registers of 1 to 20 qubits, on a deferring
// register and on views; the launch shape of a 33-qubit register; a handle used by two registers, twice, and destroyed
// after use.
// Exit code 0 = every expectation held and no sanitizer report (reports abort: -fno-sanitize-recover).
#include <cstdio>
#include <numeric>
#include <vector>

#include "driver_common.h"
#include "qsv_arith_layout.h"

namespace layout = qsv_arith_layout;

struct Made {
    qsv_arith *op = nullptr;
    int m = 0, mx = 0;
    bool identity = false;
};

static Made make(int kind, int m, int mx, uint64_t a, uint64_t c, uint64_t modulus, const std::vector<uint64_t> &table = {}) {
    Made made;
    made.m = m, made.mx = mx;
    EXPECT(qsv_arith_create(kind, m, mx, a, c, modulus, table.empty() ? nullptr : table.data(), table.size(), 0, &made.op) == QSV_OK);
    layout::Params p;
    EXPECT(layout::make_params(kind, m, mx, a, c, modulus, table.empty() ? nullptr : table.data(), table.size(), &p) == nullptr);
    made.identity = p.gather_fwd.identity;
    int k = -1, mm = -1, mmx = -1;
    EXPECT(qsv_arith_info(made.op, &k, &mm, &mmx) == QSV_OK && k == kind && mm == m && mmx == mx);
    EXPECT(qsv_arith_info(made.op, nullptr, nullptr, nullptr) == QSV_OK);
    return made;
}

// every kind at width m (source width mx), plus maps that move nothing
static std::vector<Made> all_kinds(int m, int mx) {
    const uint64_t full = 1ull << m, odd = m >= 2 ? full - 1 : 2;
    std::vector<uint64_t> xor_table(1ull << mx), perm(full);
    for (size_t x = 0; x < xor_table.size(); ++x) xor_table[x] = (x * 5 + 1) % full;
    for (uint64_t y = 0; y < full; ++y) perm[y] = (y + 3) % full;
    std::vector<Made> out;
    out.push_back(make(QSV_ARITH_ADD, m, 0, 0, 1, 0));
    out.push_back(make(QSV_ARITH_ADD, m, 0, 0, 1, odd));
    out.push_back(make(QSV_ARITH_ADD, m, 0, 0, 0, 0));                       // identity
    out.push_back(make(QSV_ARITH_MUL, m, 0, m >= 2 ? 3 : 1, 0, 0));
    out.push_back(make(QSV_ARITH_MUL, m, 0, m >= 2 ? odd - 1 : 1, 0, odd));
    out.push_back(make(QSV_ARITH_MUL, m, 0, 1, 0, 0));                       // identity
    if (mx > 0) {
        out.push_back(make(QSV_ARITH_ADD_REG, m, mx, 1, 0, 0));
        out.push_back(make(QSV_ARITH_ADD_REG, m, mx, odd - 1, 1, odd));
        out.push_back(make(QSV_ARITH_MUL_POW, m, mx, m >= 2 ? 3 : 1, 0, 0));
        out.push_back(make(QSV_ARITH_MUL_POW, m, mx, m >= 2 ? odd - 1 : 1, 0, odd));
        out.push_back(make(QSV_ARITH_XOR_LOOKUP, m, mx, 0, 0, 0, xor_table));
    }
    out.push_back(make(QSV_ARITH_PERMUTE, m, 0, 0, 0, 0, perm));
    return out;
}

static void expect_valid(qsv_state *st, const Made &made, const std::vector<int> &target, const std::vector<int> &source,
                         const std::vector<int> &controls) {
    for (int flags : {0, QSV_ARITH_INVERSE}) {
        uint64_t passes = 99;
        const unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_arith(st, made.op, target.data(), source.empty() ? nullptr : source.data(), static_cast<int>(controls.size()),
                               controls.empty() ? nullptr : controls.data(), flags, &passes) == QSV_OK);
        EXPECT(passes == (made.identity ? 0u : 1u) && qsv_stub_launches - before == passes);
        EXPECT(qsv_apply_arith(st, made.op, target.data(), source.data(), static_cast<int>(controls.size()), controls.data(), flags, nullptr) == QSV_OK);
    }
}

static void destroy_all(std::vector<Made> &maps) {
    for (Made &made : maps) EXPECT(qsv_arith_destroy(made.op) == QSV_OK);
    maps.clear();
}

int main() {
    static_assert(QSV_ARITH_INVERSE == layout::ARITH_INVERSE && QSV_ARITH_PERMUTE == layout::KIND_PERMUTE, "the header's constants are the layout's");
    // ---- create: every refusal, nothing allocated, *out cleared -------------------------------------------------------------
    {
        const std::vector<uint64_t> perm = {2, 0, 3, 1}, twice = {0, 1, 1, 2}, wide = {0, 1, 2, 4}, bits = {0, 1};
        qsv_arith *op = reinterpret_cast<qsv_arith *>(&op);
        auto refused = [&](int kind, int m, int mx, uint64_t a, uint64_t c, uint64_t modulus, const std::vector<uint64_t> *table, uint64_t len, int device = 0) {
            op = reinterpret_cast<qsv_arith *>(&op);
            const int rc = qsv_arith_create(kind, m, mx, a, c, modulus, table ? table->data() : nullptr, len, device, &op);
            return rc == QSV_EINVAL && op == nullptr && qsv_last_error()[0] != '\0';
        };
        EXPECT(qsv_arith_create(QSV_ARITH_ADD, 2, 0, 0, 1, 0, nullptr, 0, 0, nullptr) == QSV_EINVAL);
        EXPECT(refused(6, 2, 0, 0, 0, 0, nullptr, 0) && refused(-1, 2, 0, 0, 0, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_ADD, 0, 0, 0, 0, 0, nullptr, 0) && refused(QSV_ARITH_ADD, 33, 0, 0, 1, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_PERMUTE, 25, 0, 0, 0, 0, &perm, 4) && refused(QSV_ARITH_MUL, -1, 0, 1, 0, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_ADD_REG, 4, 0, 1, 0, 0, nullptr, 0) && refused(QSV_ARITH_ADD_REG, 4, 33, 1, 0, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_MUL_POW, 4, 25, 3, 0, 0, nullptr, 0) && refused(QSV_ARITH_XOR_LOOKUP, 1, 0, 0, 0, 0, &bits, 1));
        EXPECT(refused(QSV_ARITH_ADD, 4, 1, 0, 1, 0, nullptr, 0) && refused(QSV_ARITH_PERMUTE, 2, 1, 0, 0, 0, &perm, 4));
        EXPECT(refused(QSV_ARITH_ADD, 4, 0, 0, 0, 1, nullptr, 0) && refused(QSV_ARITH_ADD, 4, 0, 0, 1, 17, nullptr, 0));
        EXPECT(refused(QSV_ARITH_MUL, 32, 0, 1, 0, (1ull << 32) + 1, nullptr, 0) && refused(QSV_ARITH_PERMUTE, 2, 0, 0, 0, 4, &perm, 4));
        EXPECT(refused(QSV_ARITH_MUL, 4, 0, 16, 0, 0, nullptr, 0) && refused(QSV_ARITH_MUL, 4, 0, 15, 0, 15, nullptr, 0));
        EXPECT(refused(QSV_ARITH_ADD, 4, 0, 1, 1, 0, nullptr, 0) && refused(QSV_ARITH_ADD, 4, 0, 0, 16, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_ADD_REG, 4, 2, 1, 13, 13, nullptr, 0) && refused(QSV_ARITH_MUL, 4, 0, 3, 1, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_MUL, 4, 0, 0, 0, 0, nullptr, 0) && refused(QSV_ARITH_MUL, 4, 0, 6, 0, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_MUL_POW, 4, 3, 3, 0, 15, nullptr, 0) && refused(QSV_ARITH_MUL, 4, 0, 5, 0, 15, nullptr, 0));
        EXPECT(refused(QSV_ARITH_PERMUTE, 2, 0, 0, 0, 0, &twice, 4) && refused(QSV_ARITH_PERMUTE, 2, 0, 0, 0, 0, &wide, 4));
        EXPECT(refused(QSV_ARITH_PERMUTE, 2, 0, 0, 0, 0, &perm, 3) && refused(QSV_ARITH_XOR_LOOKUP, 1, 2, 0, 0, 0, &bits, 2));
        EXPECT(refused(QSV_ARITH_PERMUTE, 2, 0, 0, 0, 0, nullptr, 4) && refused(QSV_ARITH_XOR_LOOKUP, 1, 1, 0, 0, 0, nullptr, 0));
        EXPECT(refused(QSV_ARITH_ADD, 2, 0, 0, 1, 0, &bits, 2) && refused(QSV_ARITH_XOR_LOOKUP, 1, 1, 0, 0, 0, &perm, 2));
        EXPECT(refused(QSV_ARITH_ADD, 2, 0, 0, 1, 0, nullptr, 0, 1) && refused(QSV_ARITH_ADD, 2, 0, 0, 1, 0, nullptr, 0, -1));      // no such device
        EXPECT(qsv_arith_destroy(nullptr) == QSV_OK);
        EXPECT(qsv_arith_info(nullptr, nullptr, nullptr, nullptr) == QSV_EINVAL);
    }
    // ---- the widest accepted parameters ------------------------------------------------------------------------------------
    {
        std::vector<Made> wide;
        wide.push_back(make(QSV_ARITH_ADD, 32, 0, 0, (1ull << 32) - 1, 0));
        wide.push_back(make(QSV_ARITH_MUL, 32, 0, (1ull << 32) - 2, 0, (1ull << 32) - 1));
        wide.push_back(make(QSV_ARITH_ADD_REG, 32, 32, (1ull << 32) - 1, 7, 0));
        wide.push_back(make(QSV_ARITH_MUL_POW, 32, 12, 3, 0, (1ull << 31) - 1));
        destroy_all(wide);
    }
    // ---- apply on plain registers ---------------------------------------------------------------------------------------
    for (int n : {1, 2, 5, 6, 13, 14, 18, 20}) {
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        const int m = n >= 14 ? 4 : n >= 5 ? 2 : 1, mx = n - m >= 3 ? 2 : n - m >= 1 ? 1 : 0;
        std::vector<Made> maps = all_kinds(m, mx);
        std::vector<int> high(m), low(m), reversed(m), src_low(mx), src_high(mx);
        std::iota(high.begin(), high.end(), 0);                       // qubits 0 .. m-1: the top index bits
        for (int r = 0; r < m; ++r) low[r] = n - m + r, reversed[r] = n - 1 - r;
        for (int r = 0; r < mx; ++r) src_low[r] = n - mx + r, src_high[r] = r;
        const Made &first = maps.front();
        uint64_t passes = 99;
        unsigned long before = qsv_stub_launches;
        // ---- refusals --------------------------------------------------------------------------------------------------
        std::vector<int> bad = high;
        EXPECT(qsv_apply_arith(nullptr, first.op, high.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, nullptr, high.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, nullptr, nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, 1, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, -1, high.data(), 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, 0, nullptr, 2, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, 0, nullptr, -1, &passes) == QSV_EINVAL);
        bad[0] = n;
        EXPECT(qsv_apply_arith(st, first.op, bad.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        bad[0] = -1;
        EXPECT(qsv_apply_arith(st, first.op, bad.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, 1, &high[0], 0, &passes) == QSV_EINVAL);       // a control that is a target
        const int outside[1] = {n};
        EXPECT(qsv_apply_arith(st, first.op, high.data(), nullptr, 1, outside, 0, &passes) == QSV_EINVAL);
        if (m >= 2) {
            bad = high, bad[1] = bad[0];
            EXPECT(qsv_apply_arith(st, first.op, bad.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        }
        if (mx > 0 && n - m >= 1) {
            const Made &reg = maps[6];                                    // ADD_REG
            EXPECT(qsv_apply_arith(st, reg.op, high.data(), nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);      // source missing
            std::vector<int> overlapping = src_low;
            overlapping[0] = high[0];
            EXPECT(qsv_apply_arith(st, reg.op, high.data(), overlapping.data(), 0, nullptr, 0, &passes) == QSV_EINVAL);
            if (n - m - mx >= 1) EXPECT(qsv_apply_arith(st, reg.op, high.data(), src_low.data(), 1, &src_low[0], 0, &passes) == QSV_EINVAL);
            if (n - m - mx >= 2) {
                const int twice[2] = {m, m};
                EXPECT(qsv_apply_arith(st, reg.op, high.data(), src_low.data(), 2, twice, 0, &passes) == QSV_EINVAL);
            }
        }
        EXPECT(qsv_stub_launches == before);
        // ---- valid calls: every kind, both directions, targets high / low / reversed, sources low / high, 0 .. 2 controls -----------
        for (const Made &made : maps) {
            const bool sourced = made.mx > 0;
            expect_valid(st, made, high, sourced ? src_low : std::vector<int>{}, {});
            if (n - m - mx >= m || !sourced) {
                if (!sourced) expect_valid(st, made, low, {}, {});
                if (!sourced) expect_valid(st, made, reversed, {}, {});
            }
            if (sourced && n >= 2 * m + mx) expect_valid(st, made, low, src_high, {});
            std::vector<int> free_qubits;
            for (int q = m; q < n - (sourced ? mx : 0); ++q) free_qubits.push_back(q);
            if (free_qubits.size() >= 1) expect_valid(st, made, high, sourced ? src_low : std::vector<int>{}, {free_qubits.back()});
            if (free_qubits.size() >= 2) expect_valid(st, made, high, sourced ? src_low : std::vector<int>{}, {free_qubits.front(), free_qubits.back()});
        }
        // the whole register as the target
        if (n <= 20) {
            std::vector<uint64_t> perm(1ull << n);
            for (uint64_t y = 0; y < perm.size(); ++y) perm[y] = y ^ 1;
            std::vector<int> all(n);
            std::iota(all.begin(), all.end(), 0);
            std::vector<Made> whole = {make(QSV_ARITH_ADD, n, 0, 0, 1, 0), make(QSV_ARITH_MUL, n, 0, 1, 0, 2), make(QSV_ARITH_PERMUTE, n, 0, 0, 0, 0, perm)};
            for (const Made &made : whole) expect_valid(st, made, all, {}, {});
            destroy_all(whole);
        }
        EXPECT(qsv_destroy(st) == QSV_OK);
        destroy_all(maps);
    }
    // ---- a deferring register: a refused call leaves the queue alone, a valid one flushes it first; identity maps flush too -----
    {
        const int n = 14;
        qsv_state *st = nullptr;
        EXPECT(qsv_create(n, 0, &st) == QSV_OK);
        EXPECT(qsv_set_option(st, QSV_OPT_DEFER, 2) == QSV_OK);
        const double h[8] = {0.5, 0, 0.5, 0, 0.5, 0, -0.5, 0};
        EXPECT(qsv_apply_1q(st, 3, h) == QSV_OK);
        const Stats queued = stats_of(st);
        const unsigned long before = qsv_stub_launches;
        Made add = make(QSV_ARITH_ADD, 3, 0, 0, 5, 7);
        const int target[3] = {2, 9, 0}, bad[3] = {2, 14, 0}, control[1] = {13};
        uint64_t passes = 99;
        EXPECT(qsv_apply_arith(st, add.op, bad, nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_apply_arith(st, add.op, target, nullptr, 0, nullptr, 4, &passes) == QSV_EINVAL);
        Stats now = stats_of(st);
        EXPECT(queued.queued == 1 && now.queued == 1 && now.launched == queued.launched && qsv_stub_launches == before);
        EXPECT(qsv_apply_arith(st, add.op, target, nullptr, 1, control, 0, &passes) == QSV_OK);
        now = stats_of(st);
        EXPECT(now.launched == queued.launched + 1 && now.queued == 1);       // the queued gate went out; the map was never queued
        EXPECT(passes == 1 && qsv_stub_launches == before + 2);
        expect_valid(st, add, {2, 9, 0}, {}, {13, 5});
        EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_arith_destroy(add.op) == QSV_OK);
    }
    // ---- views on caller-owned memory (the result is copied back into it), a handle shared by two registers and used twice ----
    {
        Made pow = make(QSV_ARITH_MUL_POW, 4, 3, 7, 0, 15);
        qsv_state *views[2] = {nullptr, nullptr};
        std::vector<double> mem6(2ull << 8, 0.0), mem13(2ull << 14, 0.0);
        EXPECT(qsv_create_view(8, 0, mem6.data(), 1ull << 8, nullptr, &views[0]) == QSV_OK);
        EXPECT(qsv_create_view(14, 0, mem13.data(), 1ull << 14, nullptr, &views[1]) == QSV_OK);
        for (qsv_state *st : views) {
            const unsigned long copied = qsv_stub_bytes_copied;
            expect_valid(st, pow, {0, 1, 2, 3}, {7, 6, 5}, {});
            expect_valid(st, pow, {7, 5, 3, 1}, {0, 2, 4}, {6});
            EXPECT(qsv_stub_bytes_copied > copied);                         // the spare buffer went back into the caller's memory
            void *ptr = nullptr;
            EXPECT(qsv_device_ptr(st, &ptr) == QSV_OK && (ptr == mem6.data() || ptr == mem13.data()));
        }
        EXPECT(qsv_destroy(views[0]) == QSV_OK);
        expect_valid(views[1], pow, {0, 1, 2, 3}, {7, 6, 5}, {});           // the handle outlives a register that used it
        EXPECT(qsv_destroy(views[1]) == QSV_OK);
        EXPECT(qsv_arith_destroy(pow.op) == QSV_OK);
    }
    // ---- a mode register, and a handle on another device ----------------------------------------------------------------------
    {
        qsv_state *st = nullptr;
        EXPECT(qsv_create_qudit(3, 3, 0, &st) == QSV_OK);
        Made add = make(QSV_ARITH_ADD, 1, 0, 0, 1, 0);
        const int q[1] = {0};
        uint64_t passes = 99;
        unsigned long before = qsv_stub_launches;
        EXPECT(qsv_apply_arith(st, add.op, q, nullptr, 0, nullptr, 0, &passes) == QSV_ESTATE);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK);
        qsv_stub_devices = 2;
        qsv_arith *far = nullptr;
        EXPECT(qsv_arith_create(QSV_ARITH_ADD, 1, 0, 0, 1, 0, nullptr, 0, 1, &far) == QSV_OK);
        EXPECT(qsv_create(3, 0, &st) == QSV_OK);
        before = qsv_stub_launches;
        EXPECT(qsv_apply_arith(st, far, q, nullptr, 0, nullptr, 0, &passes) == QSV_EINVAL);
        EXPECT(qsv_stub_launches == before);
        EXPECT(qsv_destroy(st) == QSV_OK);
        EXPECT(qsv_arith_destroy(far) == QSV_OK);
        qsv_stub_devices = 1;
        EXPECT(qsv_arith_destroy(add.op) == QSV_OK);
    }
    // ---- the launch shape of a 33-qubit register: one dispatch of fewer than 2^32 work-items that strides over 2^31 work items ----
    {
        const int n = 33;
        const uint64_t tmask = 0xfull << 20;
        const layout::Shape shape = layout::launch_shape(n, tmask, layout::ARITH_MAX_ITEMS_LOG2);
        EXPECT(shape.form == layout::FORM_LINE && shape.items_log2 == 2 && shape.item_bit[0] == 6 && shape.item_bit[1] == 7);
        EXPECT(shape.W == 1ull << 31 && static_cast<uint64_t>(shape.grid) * layout::ARITH_BLOCK < 1ull << 32 && shape.grid == layout::ARITH_GRID_CAP);
        const layout::Shape low = layout::launch_shape(n, (1ull << n) - 1, 2);
        EXPECT(low.form == layout::FORM_ELEMENT && low.items_log2 == 0 && low.W == 1ull << 33 && low.grid == layout::ARITH_GRID_CAP);
        const layout::Shape one = layout::launch_shape(n, tmask, layout::ARITH_DEFAULT_ITEMS_LOG2);      // what the library launches
        EXPECT(one.items_log2 == 0 && one.W == 1ull << 33 && static_cast<uint64_t>(one.grid) * layout::ARITH_BLOCK == 1ull << 28);
    }
    return finish("register-arithmetic");
}

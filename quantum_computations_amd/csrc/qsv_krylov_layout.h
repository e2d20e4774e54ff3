// Host-side layouts of the multi-register BLAS-1 launchers (qsv_krylov.hip: qsv_lincomb, qsv_inner_many): plain C++, no
// HIP, so that the host tests can compile it alone (tests/test_krylov_layout_host.py).
//
// Both calls cut their operand list into passes of at most KRYLOV_OPERANDS_PER_PASS registers.  A pass streams its
// operands once; what it reduces (the inner products, the squared norm of what qsv_lincomb stores) leaves the kernel as
// one complex partial per workgroup and slot in a slice of the scratch buffer, and the host sums a slot's partials in
// index order.  Everything here is index arithmetic.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qsv_krylov_layout {

constexpr int KRYLOV_OPERANDS_PER_PASS = 8;
constexpr int KRYLOV_BLOCK = 256;             // = QSV_BLOCK
constexpr int KRYLOV_REDUCE_BLOCKS = 1024;    // = QSV_REDUCE_BLOCKS
constexpr uint64_t KRYLOV_MAX_BLOCKS = 0x00ffffffull;   // an AQL dispatch counts work-items in 32 bits (grid_for)

// ---- argument types of the kernels (passed by value: field order and sizes are ABI) -------------------------------------

// k_lincomb<K, BETA, NORM, NT>: dst = beta dst + sum_{k < K} c[k] src[k]; only the first K slots are ever read.
struct LincombArgs {
    uint64_t amps;
    double beta_re, beta_im;
    double c_re[KRYLOV_OPERANDS_PER_PASS];
    double c_im[KRYLOV_OPERANDS_PER_PASS];
    const void *src[KRYLOV_OPERANDS_PER_PASS];
};
static_assert(sizeof(LincombArgs) == 24 + 24 * KRYLOV_OPERANDS_PER_PASS, "kernel argument layout");

// k_inner_many<K>: partials of <x[k] | y>, k < K.
struct InnerManyArgs {
    uint64_t amps;
    const void *x[KRYLOV_OPERANDS_PER_PASS];
};
static_assert(sizeof(InnerManyArgs) == 8 + 8 * KRYLOV_OPERANDS_PER_PASS, "kernel argument layout");

// ---- grids --------------------------------------------------------------------------------------------------------------
inline int blocks_for(uint64_t amps, uint64_t cap) {
    uint64_t blocks = (amps + KRYLOV_BLOCK - 1) / KRYLOV_BLOCK;
    blocks = std::max<uint64_t>(blocks, 1);
    if (cap > 0) blocks = std::min(blocks, cap);
    return static_cast<int>(std::min(blocks, KRYLOV_MAX_BLOCKS));
}
// A pass that reduces writes one partial per workgroup: at most KRYLOV_REDUCE_BLOCKS workgroups, fewer where
// QSV_OPT_GRID_CAP (grid_cap > 0) says so.  Its threads loop from 2^18 amplitudes on.
inline int reduce_grid(uint64_t amps, int grid_cap) {
    const uint64_t cap = grid_cap > 0 ? std::min<uint64_t>(grid_cap, KRYLOV_REDUCE_BLOCKS) : KRYLOV_REDUCE_BLOCKS;
    return blocks_for(amps, cap);
}
// A pass that only streams: one amplitude per thread, as the other register-moving kernels (grid_cap = 0: no cap but the
// dispatch limit, so the loop runs more than once beyond 2^32 amplitudes only).
inline int stream_grid(uint64_t amps, int grid_cap) { return blocks_for(amps, grid_cap > 0 ? static_cast<uint64_t>(grid_cap) : 0); }

// ---- qsv_lincomb --------------------------------------------------------------------------------------------------------
struct LincombPass {
    int first = 0, count = 0;      // sources [first, first + count) of the caller's list; count = 0: scale or zero dst
    double beta_re = 0.0, beta_im = 0.0;
    bool reads_dst = false;        // beta != 0: the pass loads the old dst
    bool norm = false;             // the last pass of a call that wants ||dst||^2
    int grid = 0;
    size_t partial_offset = 0;     // doubles into the scratch buffer (norm only): grid x {re, im = 0}
};
// n_src sources -> max(1, ceil(n_src / 8)) passes.  The first carries the caller's beta, the others beta = 1; only the
// last forms the norm.
inline std::vector<LincombPass> lincomb_passes(int n_src, double beta_re, double beta_im, bool want_norm, uint64_t amps, int grid_cap) {
    std::vector<LincombPass> out;
    const int passes = std::max(1, (n_src + KRYLOV_OPERANDS_PER_PASS - 1) / KRYLOV_OPERANDS_PER_PASS);
    for (int p = 0; p < passes; ++p) {
        LincombPass a;
        a.first = p * KRYLOV_OPERANDS_PER_PASS;
        a.count = std::min(KRYLOV_OPERANDS_PER_PASS, n_src - a.first);
        a.beta_re = p == 0 ? beta_re : 1.0;
        a.beta_im = p == 0 ? beta_im : 0.0;
        a.reads_dst = !(a.beta_re == 0.0 && a.beta_im == 0.0);
        a.norm = want_norm && p == passes - 1;
        a.grid = a.norm ? reduce_grid(amps, grid_cap) : stream_grid(amps, grid_cap);
        out.push_back(a);
    }
    return out;
}
// coeffs: the caller's n_src interleaved complex coefficients; srcs: the sources' device addresses.
inline LincombArgs lincomb_args(const LincombPass &p, uint64_t amps, const double *coeffs, const void *const *srcs) {
    LincombArgs g = {};
    g.amps = amps;
    g.beta_re = p.beta_re;
    g.beta_im = p.beta_im;
    for (int k = 0; k < p.count; ++k) {
        g.c_re[k] = coeffs[2 * (p.first + k)];
        g.c_im[k] = coeffs[2 * (p.first + k) + 1];
        g.src[k] = srcs[p.first + k];
    }
    return g;
}

// ---- qsv_inner_many -----------------------------------------------------------------------------------------------------
struct InnerPass {
    int first = 0, count = 0;      // x[first .. first + count) of the caller's list, 1 .. 8
    int grid = 0;
    size_t partial_offset = 0;     // doubles into the scratch buffer: [block][slot < count]{re, im}
};
struct InnerPlan {
    std::vector<InnerPass> passes;
    size_t doubles = 0;            // of the scratch buffer, all passes
};
inline InnerPlan inner_plan(int n_x, uint64_t amps, int grid_cap) {
    InnerPlan plan;
    for (int first = 0; first < n_x; first += KRYLOV_OPERANDS_PER_PASS) {
        InnerPass a;
        a.first = first;
        a.count = std::min(KRYLOV_OPERANDS_PER_PASS, n_x - first);
        a.grid = reduce_grid(amps, grid_cap);
        a.partial_offset = plan.doubles;
        plan.doubles += static_cast<size_t>(a.grid) * a.count * 2;
        plan.passes.push_back(a);
    }
    return plan;
}
inline InnerManyArgs inner_args(const InnerPass &p, uint64_t amps, const void *const *xs) {
    InnerManyArgs g = {};
    g.amps = amps;
    for (int k = 0; k < p.count; ++k) g.x[k] = xs[p.first + k];
    return g;
}
// values[2 (first + k)], [.. + 1] = the sum over the pass's workgroups, in index order.
inline void inner_sum(const InnerPass &p, const double *host, double *values) {
    for (int k = 0; k < p.count; ++k) {
        double sr = 0.0, si = 0.0;
        for (int b = 0; b < p.grid; ++b) {
            sr += host[p.partial_offset + (static_cast<size_t>(b) * p.count + k) * 2];
            si += host[p.partial_offset + (static_cast<size_t>(b) * p.count + k) * 2 + 1];
        }
        values[2 * (p.first + k)] = sr;
        values[2 * (p.first + k) + 1] = si;
    }
}

}  // namespace qsv_krylov_layout

// Internal, host only (plain C++17, no HIP types): every decision of the MPS splits that fixes the kept rank or the route
// a matrix takes -- the truncation rule, the acceptance tests of the zgesdd and the verified low-rank routes, the route
// choice of the exact split, the dust floor of the whole-matrix Jacobi sweeps, the share plan of the skinny products and
// the environment switches.  tests/layout/split_rules_driver.cpp exercises them without a GPU.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace qsv_split_rules {

constexpr int JACOBI_MAX_COLUMNS = 2048;      // widest short side the whole-matrix Jacobi sweeps take
constexpr int SKINNY_SLAB = 32;               // summed-dimension values per LDS slab of the skinny products
constexpr unsigned SKINNY_MAX_SHARES = 16;

// ---- the environment switches ("Runtime switches"), read once per process ----------------------------
struct SplitOptions {
    bool shortcuts = true;      // QSV_SVD != exact: the verified low-rank route and zgesdd may answer the exact split
    bool jacobi = true;         // QSV_SVD != exact, != library: whole-matrix Jacobi sweeps before zgesvd
    bool fused_panels = true;   // QSV_RSVD != rocsolver: MFMA panel products, CholeskyQR3 panels, Jacobi factor SVD
    int svd_threads = 256;      // QSV_SVD_THREADS = 512 | 1024: workgroup size of k_small_svd
    int panel_rounds = 2;       // QSV_PANEL_ROUNDS = 3: CholeskyQR rounds of the intermediate panels
    bool trace = false;         // QSV_TRACE_SPLIT set: decisions of the splits on stderr
};

inline SplitOptions parse_split_options(const char *svd, const char *rsvd, const char *threads, const char *rounds,
                                        const char *trace) {
    SplitOptions o;
    const std::string s = svd ? svd : "";
    o.shortcuts = s != "exact";
    o.jacobi = s != "exact" && s != "library";
    o.fused_panels = !(rsvd && std::string(rsvd) == "rocsolver");
    const int n = threads ? atoi(threads) : 256;
    o.svd_threads = n == 512 || n == 1024 ? n : 256;
    o.panel_rounds = rounds && atoi(rounds) == 3 ? 3 : 2;
    o.trace = trace != nullptr;
    return o;
}

inline const SplitOptions &split_options() {
    static const SplitOptions o = parse_split_options(std::getenv("QSV_SVD"), std::getenv("QSV_RSVD"), std::getenv("QSV_SVD_THREADS"),
                                                      std::getenv("QSV_PANEL_ROUNDS"), std::getenv("QSV_TRACE_SPLIT"));
    return o;
}

// ---- the reference's truncation rule (mps.py:83-86) on singular values sorted in decreasing order --------------------
inline double allowed_error(const std::vector<double> &sv, double abs_err, double rel_err) {
    double total = 0.0;
    for (double v : sv) total += v;
    double allowed = total * rel_err;
    if (abs_err > allowed) allowed = abs_err;
    return allowed < 0.0 ? 0.0 : allowed;
}

inline uint64_t kept_rank_for(const std::vector<double> &sv, int64_t max_bond_dim, double allowed) {
    uint64_t r = 0;
    double tail = 0.0;
    for (size_t i = sv.size(); i-- > 0;) {
        tail += sv[i];
        if (tail > allowed) ++r;
    }
    if (max_bond_dim >= 0 && r > static_cast<uint64_t>(max_bond_dim)) r = static_cast<uint64_t>(max_bond_dim);
    if (r > sv.size()) r = sv.size();
    return r;
}

inline uint64_t kept_rank(const std::vector<double> &sv, int64_t max_bond_dim, double abs_err, double rel_err) {
    return kept_rank_for(sv, max_bond_dim, allowed_error(sv, abs_err, rel_err));
}

// ---- the exact split: which routes a (rows x cols) theta may take ----------------------------------------------------
struct ExactRoute {
    bool hopeless;      // an absolute tolerance far below the scale of theta: zgesdd cannot pass its test
    bool loose;         // zgesdd's answer may be tried as it is: the tolerance might not tell the difference
    bool jacobi_fits;   // the whole-matrix Jacobi sweeps take this shape
};

// `frobenius2` = ||theta||_F^2, or <= 0 when nobody measured it
inline ExactRoute exact_route(uint64_t rows, uint64_t cols, double abs_err, double rel_err, double frobenius2,
                              const SplitOptions &o) {
    ExactRoute route{false, false, false};
    const uint64_t k = rows < cols ? rows : cols;
    if (frobenius2 > 0.0) {
        const double norm = sqrt(frobenius2);
        route.hopeless = (abs_err > rel_err * norm ? abs_err : rel_err * norm) < 1e-5 * norm;
    }
    // zgesdd's answer is tried as it is only when the tolerance cannot tell the difference; under a tight one its factors
    // still seed the Jacobi sweeps over the whole matrix (jacobi_full_split), which then need a handful of sweeps
    route.loose = !route.hopeless && (rel_err >= 1e-6 || abs_err > 0.0);
    // (sweeps move the whole working matrix once per tournament step: beyond 2^26 amplitudes the library is no slower)
    route.jacobi_fits = o.jacobi && k >= 2 && k <= static_cast<uint64_t>(JACOBI_MAX_COLUMNS) && rows * cols <= (1ull << 26);
    return route;
}

// rocSOLVER's zgesdd goes through the eigenvectors of A^H A and cannot resolve singular values below ~1e-8 sigma_max.
// Its values `sv` decide the split when the truncation cannot notice: the allowed error must exceed the possible garbage
// in the tail sum by a wide margin, the kept rank must be the same at both ends of that margin, and every kept value
// must be well above the floor.
inline bool gram_values_decide(const std::vector<double> &sv, int64_t max_bond_dim, double abs_err, double rel_err) {
    if (sv.empty()) return false;
    const double floor_value = 2e-8 * sv[0], margin = floor_value * static_cast<double>(sv.size());
    const double allowed = allowed_error(sv, abs_err, rel_err);
    if (!(allowed > 100.0 * margin)) return false;
    const uint64_t r_lo = kept_rank_for(sv, max_bond_dim, allowed + margin);
    const uint64_t r_hi = kept_rank_for(sv, max_bond_dim, allowed - margin);
    return r_lo == r_hi && (r_lo == 0 || sv[r_lo - 1] > 1e3 * floor_value);
}

// ---- whole-matrix Jacobi sweeps on L-entry columns: rounding dust ------------------------------------------------------
// Columns of norm below 4 sqrt(L) eps ||X||_F are rounding dust (the product X J itself is only that accurate): the
// squared norm below which a column sits out of the sweeps and is relabelled afterwards.
inline double dust_floor2(uint64_t L, double frobenius2) {
    return 16.0 * static_cast<double>(L) * 4.930380657631324e-32 * frobenius2;
}

// `norm2`: squared column norms after the sweeps, sorted decreasingly; returns their square roots.  The norm of a dust
// column is the rounding error of the product X J (hundreds of eps sigma_max), not a singular value; a backward-stable SVD
// reports eps sigma_max-sized values there, and a tail of 500 such columns must not reach a tight truncation threshold.
// Dust is relabelled to at most eps sigma_max, in `norm2` too (*relabelled says whether any was).
inline std::vector<double> values_from_norms(std::vector<double> &norm2, double floor2, bool *relabelled) {
    std::vector<double> sv(norm2.size());
    for (size_t c = 0; c < sv.size(); ++c) sv[c] = sqrt(norm2[c]);
    *relabelled = false;
    for (size_t c = 0; c < sv.size(); ++c)
        if (!(norm2[c] > floor2)) {
            const double label = sv[c] < 2.220446049250313e-16 * sv[0] ? sv[c] : 2.220446049250313e-16 * sv[0];
            sv[c] = label;
            norm2[c] = label * label;
            *relabelled = true;
        }
    return sv;
}

// ---- the verified low-rank route: is the kept rank settled by the l computed values `sv`? -----------------------------
// What the projection misses: rho^2 = ||A||_F^2 - sum sigma~_i^2 = ||(I - Q Q^H) A||_F^2 exactly.  With
// d_i = sigma_i^2 - sigma~_i^2 >= 0 (i <= l; singular values of a compression never exceed the true ones) and
// d_i = sigma_i^2 (i > l) one has sum d_i = rho^2 and sigma_i - sigma~_i <= sqrt(d_i), so every true tail sum lies
// in [T~_j, T~_j + sqrt(full) rho] (Cauchy-Schwarz).
struct LowRankVerdict {
    bool settled;       // the truncation rule gives rank `r` on the full spectrum too
    uint64_t r;
    bool compared;      // the two thresholds were evaluated: r_lo, r_hi are meaningful
    double rho, margin, allowed;
    uint64_t r_lo, r_hi;
};

// `rho2_bound` bounds the missed mass; `k_keep` = how many of the computed triplets may be kept
inline LowRankVerdict low_rank_settled(const std::vector<double> &sv, double rho2_bound, uint64_t full_rank, int64_t max_bond_dim,
                                       int64_t k_keep, double abs_err, double rel_err) {
    LowRankVerdict v{false, 0, false, sqrt(rho2_bound), 0.0, allowed_error(sv, abs_err, rel_err), 0, 0};
    v.margin = sqrt(static_cast<double>(full_rank)) * v.rho;
    if (!(v.allowed > v.margin)) return v;
    // true tail sums are the computed ones plus something in [0, margin]; the true allowance is the computed one
    // plus at most rel_err * margin: the rank is settled if no computed tail sum falls between these two thresholds
    v.r_lo = kept_rank_for(sv, max_bond_dim, v.allowed + rel_err * v.margin);
    v.r_hi = kept_rank_for(sv, max_bond_dim, v.allowed - v.margin);
    v.compared = true;
    // the kept triplets must sit well inside the captured block and far above what was missed (their subspace
    // error after q power iterations is of order (rho / sigma_r)^(2q+1))
    if (v.r_lo != v.r_hi || v.r_lo > static_cast<uint64_t>(k_keep) || (v.r_lo > 0 && !(sv[v.r_lo - 1] > 1e2 * v.rho))) return v;
    v.settled = true;
    v.r = v.r_lo;
    return v;
}

// ---- split-K of a skinny product with `out_rows` output rows, `l` <= 64 columns and `depth` summed values ------------
struct SharePlan {
    unsigned split;     // shares of the summed dimension (gridDim.y)
    bool shares;        // each share writes its own copy (summed in order afterwards) instead of atomic adds into Y
};

// One wave per SIMD cannot hide its own load latency: below two workgroups per CU the range is cut in two (the two partial
// sums meet in a zero-initialised Y through atomic adds: a + b does not depend on which arrives first) -- or, with a
// workspace of `share_amps` amplitudes, into as many shares as give every CU two workgroups, each at least four slabs deep.
inline SharePlan skinny_share_plan(uint64_t out_rows, uint64_t depth, int l, uint64_t share_amps) {
    const unsigned row_blocks = static_cast<unsigned>((out_rows + 63) / 64);
    SharePlan plan{row_blocks < 512 && depth >= 4 * SKINNY_SLAB ? 2u : 1u, false};
    if (plan.split > 1 && share_amps && row_blocks < 256) {
        unsigned want = (512 + row_blocks - 1) / row_blocks;
        const uint64_t deepest = depth / (4 * SKINNY_SLAB);
        if (want > SKINNY_MAX_SHARES) want = SKINNY_MAX_SHARES;
        if (want > deepest) want = static_cast<unsigned>(deepest);
        while (want > 2 && static_cast<uint64_t>(want) * out_rows * l > share_amps) --want;
        if (want > 2) plan = SharePlan{want, true};
    }
    return plan;
}

}  // namespace qsv_split_rules

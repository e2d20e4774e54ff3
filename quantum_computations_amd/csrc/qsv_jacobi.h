// Internal: the one-sided Jacobi step shared by the four SVD kernels -- the pair schedule (host and device) and the device
// helpers for one column pair (x = column p, y = column q):
//     alpha = |x|^2, beta = |y|^2, gamma = x^H y;   y <- y conj(gamma / |gamma|);   (x, y) <- (c x - s y, s x + c y).
// Each kernel keeps its own "rotate or not" condition at the call site, next to the comment that justifies it:
//
//   kernel                         rotates when                                         why
//   k_small_svd    (qsv_panel)     g2 > eps^2 alpha beta, g2 > 0                        columns of <= 64 entries in LDS: the plain rounding level
//   k_jacobi_step  (qsv_panel)     g2 > eps^2 alpha beta, g2 > 0                        the same sweeps on factors of up to 256 columns
//   k_jacobi_pair  (qsv_decomp)    g2 > L eps^2 alpha beta, g2 > 0, alpha, beta above   columns of L (thousands of) entries: gamma is noise below
//                                  the dust floor                                       sqrt(L) eps; dust columns would keep the sweeps going
//   k_site_jacobi  (qsv_canonical) |gamma| (hypot) > eps sqrt(alpha) sqrt(beta), the     null columns of a rank-deficient Gram matrix reach the
//                                  shorter column > 1e-40 of the longer (squared)       underflow range, where g2 and the phase lose their meaning
// (g2 = |gamma|^2, eps = 2^-52.)
#pragma once

#if defined(__HIPCC__)
#include "qsv_internal.h"
#define QSV_JACOBI_HD __host__ __device__ __forceinline__
#else
#define QSV_JACOBI_HD inline
#endif

namespace qsv_jacobi {

// Round-robin tournament over lp (even) columns: step 0 .. lp-2 pairs every column once, lp / 2 disjoint pairs per step;
// pair 0 .. lp/2-1 of a step is (p, q) with p < q.  An odd number of columns l = lp - 1 is padded: the pair with q >= l sits out.
struct ColumnPair {
    int p, q;
};
// (returned by value: written through two references the schedule compiles differently inside k_small_svd and k_site_jacobi)
QSV_JACOBI_HD ColumnPair tournament_pair(int lp, int step, int pair) {
    int p, q;
    if (pair == 0) {
        p = lp - 1;
        q = step;
    } else {
        p = (step + pair) % (lp - 1);
        q = (step - pair + (lp - 1)) % (lp - 1);
    }
    if (p > q) {
        const int tmp = p;
        p = q;
        q = tmp;
    }
    return ColumnPair{p, q};
}

#if defined(__HIPCC__)
constexpr double EPS = 2.220446049250313e-16;

__device__ __forceinline__ amp_t conj_mul(amp_t a, amp_t b) {   // conj(a) * b
    return amp_t{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ amp_t plain_mul(amp_t a, amp_t b) {
    return amp_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}

// The sums of one column pair, kept by the kernels as `double alpha, beta; amp_t gamma`.  QSV_JACOBI_ACCUMULATE adds one
// entry pair (x of column p, y of column q); QSV_JACOBI_TEAM_REDUCE sums over an aligned group of `team` lanes (a power
// of two; 64 = the wave) by butterfly exchanges, and every lane of the group ends with the group's sums.  Statement macros,
// not functions: through a function (by reference, by value or as a struct) the compiler simplifies these lines before
// they meet the kernel, and k_jacobi_step, k_small_svd and k_site_jacobi then come out with reordered instructions;
// expanded in place all four kernels compile to the code they had when each wrote the lines out (tools/device_code_diff.py).
#define QSV_JACOBI_ACCUMULATE(alpha, beta, gamma, x, y)                \
    do {                                                               \
        alpha += (x).x * (x).x + (x).y * (x).y;                        \
        beta += (y).x * (y).x + (y).y * (y).y;                         \
        const amp_t g_ = qsv_jacobi::conj_mul(x, y);                   \
        gamma.x += g_.x;                                               \
        gamma.y += g_.y;                                               \
    } while (0)
#define QSV_JACOBI_TEAM_REDUCE(alpha, beta, gamma, team)               \
    do {                                                               \
        for (int o_ = (team) / 2; o_ > 0; o_ >>= 1) {                  \
            alpha += __shfl_xor(alpha, o_, 64);                        \
            beta += __shfl_xor(beta, o_, 64);                          \
            gamma.x += __shfl_xor(gamma.x, o_, 64);                    \
            gamma.y += __shfl_xor(gamma.y, o_, 64);                    \
        }                                                              \
    } while (0)

struct Rotation {
    amp_t phase;      // conj(gamma / |gamma|)
    double c, sn;
};

// `g` = |gamma| as the caller computed it (sqrt of g2, or hypot)
__device__ __forceinline__ Rotation rotation_for(double alpha, double beta, amp_t gamma, double g) {
    const amp_t phase = {gamma.x / g, -gamma.y / g};
    const double zeta = (beta - alpha) / (2.0 * g);
    const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + tt * tt), sn = c * tt;
    return Rotation{phase, c, sn};
}

__device__ __forceinline__ void rotate(amp_t &xp, amp_t &yq, const Rotation &rot) {
    const amp_t x = xp, y = plain_mul(yq, rot.phase);
    xp = amp_t{rot.c * x.x - rot.sn * y.x, rot.c * x.y - rot.sn * y.y};
    yq = amp_t{rot.sn * x.x + rot.c * y.x, rot.sn * x.y + rot.c * y.y};
}

// rank (an int of the caller's) = position of column c when the l columns are ordered by decreasing sigma (ties: the
// lower index first); a statement macro for the same reason as the two above (k_jacobi_finish)
#define QSV_JACOBI_RANK(rank, sigma, l, c)                                                                             \
    do {                                                                                                               \
        rank = 0;                                                                                                      \
        for (int o_ = 0; o_ < (l); ++o_) rank += sigma[o_] > sigma[c] || (sigma[o_] == sigma[c] && o_ < (c));         \
    } while (0)
#endif

}  // namespace qsv_jacobi

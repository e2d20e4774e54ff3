// Orthogonalising one site of a matrix-product state (SiteRegister.canonicalise / compress): qsv_tensor_site_orthogonalise.
//
// The site is read as it is stored (row-major complex128): for side 0 as the tall matrix M (N x w), N = L d, w = R, for
// side 1 as the wide matrix M (w x N), w = L, N = d R.  Both are written below as the side-0 problem X = Q B with X = M
// resp. X = M^H (N x w), Q (N x w) with orthonormal columns and B (w x w) small; side 1 conjugates on the fly and never
// builds X.
//
// Route: three rounds of "Gram matrix -> Hermitian Jacobi -> scale", a rank-revealing variant of shifted CholeskyQR3 in
// which the triangular factor is replaced by the eigen-decomposition G = V diag(lambda) V^H, so that equal columns, zero
// columns and bonds wider than N need no pivoting:
//     round 1   G = X^H X;  s_j = sqrt(max(lambda_j, delta lambda_0));   Q1 = X V diag(1/s)        (nothing dropped: what
//               the Gram matrix cannot resolve -- singular values below sqrt(delta) s_0 -- is only scaled up by a bounded factor)
//     round 2   G = Q1^H Q1 resolves those directions too (they now have norm <= 1 next to the resolved ones at 1);
//               directions with lambda_j < 4 delta lambda_0 are numerically absent (singular value below ~2 delta s_0 of X)
//               and are dropped: their column of the scaling matrix is zero
//     round 3   G = Q2^H Q2 is the identity to O(1/4) on the kept directions: one more step takes it to rounding level
// with delta = 8 eps max(w, sqrt(N)), the size of the rounding of a Gram sum over N rows.  The small factor
// B = diag(s3) V3^H diag(s2) V2^H diag(s1) V1^H is accumulated explicitly as W = B^H; a one-sided Jacobi SVD of W (every Jacobi result is polished by one Newton-Schulz
// step, which takes the rotations' J^H J - 1 from several 1e-15 to the rounding of one product),
// W J = U diag(sigma), gives the singular values sigma of the site matrix (absolute accuracy O(delta) sigma_0, like a
// backward-stable dense SVD; no relative accuracy is claimed for values below sqrt(eps) sigma_0), iso = Q3 J and
// carry = diag(sigma) U^H (side 0) resp. U diag(sigma) (side 1).  The last rotation is folded into round 3's scaling
// matrix, so the big operand is read six times and written three times in all.
//
// Hot kernels (v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D col = lane & 15,
// row = (lane >> 4) + 4 reg; four real MFMAs per complex product):
//   k_site_gram<SIDE>   a wave owns one 16-row strip of G and four of its 16-column tiles, and a contiguous share of the
//                       N rows; both operands are the same per-lane loads of the site.  Every wave writes its partial
//                       tiles, k_site_gram_reduce adds them in wave order: the order of every sum is a function of
//                       (N, w, side) alone, so equal inputs give equal bits on any stream, whatever else runs.
//   k_site_apply<SIDE>  Q' = Q T (side 0) resp. T' Q (side 1): a wave owns 32 long-index positions and up to 64 columns of
//                       T, which it reads from L2 (T is at most 256 KiB).
// The small factors (w <= 128) are worked on by single-workgroup Jacobi kernels in global memory (L2-resident).
//
// Self-contained: no other translation unit refers to a symbol of this file.  Workspace comes from the grow-only pool of
// the (device, stream) context; the call ends with a synchronisation of its stream, as the pool's contract requires.
#include <cmath>

#include "qsv_jacobi.h"
#include "qsv_linalg.h"

using namespace qsvl;
using namespace qsv_jacobi;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SITE_MAX_BOND = QSV_SITE_MAX_BOND;
constexpr int GRAM_MAX_CHUNKS = 32;       // workgroups along N: 128 partial sums at most
constexpr int JACOBI_THREADS = 1024;

// element (long index n, bond index c) of the stored site
template <int SIDE>
__device__ __forceinline__ amp_t site_at(const amp_t *__restrict__ M, uint64_t N, uint64_t w, uint64_t n, uint64_t c) {
    if (n >= N || c >= w) return amp_t{0.0, 0.0};
    return SIDE == 0 ? M[n * w + c] : M[c * N + n];
}

// partials[g][a][b] = sum over the rows of wave g of conj(x[n, a]) x[n, b], x = the stored site (side 1: the conjugate of
// the Gram matrix wanted, k_site_gram_reduce flips the sign).  grid (T, ceil(T / 4), chunks), T = ceil(w / 16).
template <int SIDE>
__global__ __launch_bounds__(256) void k_site_gram(const amp_t *__restrict__ M, uint64_t N, uint64_t w,
                                                  amp_t *__restrict__ partials, unsigned wp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const unsigned ti = blockIdx.x, tj0 = 4 * blockIdx.y;
    const uint64_t g = static_cast<uint64_t>(blockIdx.z) * 4 + wave, waves = static_cast<uint64_t>(gridDim.z) * 4;
    const uint64_t steps = (N + 15) / 16;
    const uint64_t s_begin = steps * g / waves, s_end = steps * (g + 1) / waves;
    f64x4 cre[4], cim[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cre[q] = cim[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint64_t s = s_begin; s < s_end; ++s) {
        amp_t xa[4], xb[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t n = 16 * s + 4 * lk + u;       // the same k order on both operands
            xa[u] = site_at<SIDE>(M, N, w, n, 16 * ti + li);
#pragma unroll
            for (int q = 0; q < 4; ++q) xb[u][q] = site_at<SIDE>(M, N, w, n, 16 * (tj0 + q) + li);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cre[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u].x, xb[u][q].x, cre[q], 0, 0, 0);
                cim[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u].x, xb[u][q].y, cim[q], 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cre[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u].y, xb[u][q].y, cre[q], 0, 0, 0);
                cim[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[u].y, xb[u][q].x, cim[q], 0, 0, 0);
            }
        }
    }
    amp_t *out = partials + g * wp * wp;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned b = 16 * (tj0 + q) + li;
        if (b >= wp) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const unsigned a = 16 * ti + lk + 4 * reg;
            out[static_cast<uint64_t>(a) * wp + b] = amp_t{cre[q][reg], cim[q][reg]};
        }
    }
}

// G (column-major w x w) = sum of the partials in wave order; im_sign = -1 conjugates (side 1)
__global__ __launch_bounds__(256) void k_site_gram_reduce(const amp_t *__restrict__ partials, unsigned count, unsigned w,
                                                         unsigned wp, double im_sign, amp_t *__restrict__ G) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * w) return;
    const unsigned b = e / w, a = e % w;
    double re = 0.0, im = 0.0;
    for (unsigned g = 0; g < count; ++g) {
        const amp_t v = partials[(static_cast<uint64_t>(g) * wp + a) * wp + b];
        re += v.x;
        im += v.y;
    }
    G[e] = amp_t{re, im_sign * im};
}

// SIDE 0: Out (N x k) = Q (N x w) . T (w x k);  SIDE 1: Out (k x N) = T (k x w) . Q (w x N); all row-major.
// grid (ceil(N / 128), ceil(k / 64)); a wave owns two 16-wide tiles of the long index and four 16-wide tiles of k.
template <int SIDE>
__global__ __launch_bounds__(256) void k_site_apply(const amp_t *__restrict__ Q, const amp_t *__restrict__ T,
                                                   amp_t *__restrict__ Out, uint64_t N, uint64_t w, uint64_t k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const uint64_t n0 = static_cast<uint64_t>(blockIdx.x) * 128 + wave * 32;
    const uint64_t j0 = static_cast<uint64_t>(blockIdx.y) * 64;
    f64x4 cre[2][4], cim[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) cre[r][q] = cim[r][q] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint64_t c0 = 0; c0 < w; c0 += 16) {
        amp_t big[4][2], small[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t c = c0 + 4 * lk + u;
#pragma unroll
            for (int r = 0; r < 2; ++r) big[u][r] = site_at<SIDE>(Q, N, w, n0 + 16 * r + li, c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t j = j0 + 16 * q + li;
                amp_t v = amp_t{0.0, 0.0};
                if (c < w && j < k) v = SIDE == 0 ? T[c * k + j] : T[j * w + c];
                small[u][q] = v;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // the operand that carries the output row goes first: the long index (side 0) or k (side 1)
                    const amp_t a = SIDE == 0 ? big[u][r] : small[u][q], b = SIDE == 0 ? small[u][q] : big[u][r];
                    cre[r][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, cre[r][q], 0, 0, 0);
                    cim[r][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, cim[r][q], 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const amp_t a = SIDE == 0 ? big[u][r] : small[u][q], b = SIDE == 0 ? small[u][q] : big[u][r];
                    cre[r][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, cre[r][q], 0, 0, 0);
                    cim[r][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, cim[r][q], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const amp_t v = amp_t{cre[r][q][reg], cim[r][q][reg]};
                if (SIDE == 0) {
                    const uint64_t n = n0 + 16 * r + lk + 4 * reg, j = j0 + 16 * q + li;
                    if (n < N && j < k) Out[n * k + j] = v;
                } else {
                    const uint64_t j = j0 + 16 * q + lk + 4 * reg, n = n0 + 16 * r + li;
                    if (n < N && j < k) Out[j * N + n] = v;
                }
            }
}

// One-sided Jacobi on the columns of the column-major l x l matrix A (copied to the work matrix W), one workgroup:
// A J = U diag(sigma).  Column pairs follow a round-robin tournament (as k_small_svd of qsv_panel.hip, which holds its
// matrices in LDS and stops at 64 columns; here they stay in global memory, where 128 x 128 fits the L2).  Output: Js,
// the accumulated rotations with their columns sorted by decreasing sigma.  For a Hermitian positive semi-definite A
// the columns of Js are its eigenvectors.  The caller polishes Js and forms A Js itself (see `jacobi` below).
// *unconverged != 0: the 60 sweeps allowed did not end the rotations (never met; the entry point fails with QSV_EHIP).
__global__ __launch_bounds__(JACOBI_THREADS) void k_site_jacobi(const amp_t *A, amp_t *W, int l, amp_t *J, amp_t *Js,
                                                               int *unconverged) {
    __shared__ double sigma[SITE_MAX_BOND];
    __shared__ int order[SITE_MAX_BOND];
    __shared__ int rotated;
    const int t = threadIdx.x, NT = blockDim.x;
    for (int e = t; e < l * l; e += NT) {
        W[e] = A[e];
        J[e] = amp_t{e / l == e % l ? 1.0 : 0.0, 0.0};
    }
    const int lp = (l + 1) & ~1, pairs = lp / 2;
    int team = 1;                       // threads per pair: a power of two, pairs * team <= blockDim.x, team <= 64
    while (team * 2 * pairs <= NT && team < 64) team *= 2;
    const int pair = t / team, member = t % team;
    for (int sweep = 0; sweep < 60; ++sweep) {
        __syncthreads();
        if (t == 0) rotated = 0;
        for (int step = 0; step < lp - 1; ++step) {
            __syncthreads();
            int p = -1, q = -1;
            if (pair < pairs) {
                const ColumnPair cp = tournament_pair(lp, step, pair);
                p = cp.p;
                q = cp.q;
            }
            const bool live = pair < pairs && q < l;     // the padding column of an odd l sits out
            double alpha = 0.0, beta = 0.0;
            amp_t gamma = {0.0, 0.0};
            if (live)
                for (int r = member; r < l; r += team) {
                    const amp_t x = W[p * l + r], y = W[q * l + r];
                    QSV_JACOBI_ACCUMULATE(alpha, beta, gamma, x, y);
                }
            QSV_JACOBI_TEAM_REDUCE(alpha, beta, gamma, team);    // teams are aligned sub-groups of a wave
            // a column 1e-20 times shorter than its partner is rounding of the partner's own arithmetic (the null columns of
            // a rank-deficient Gram matrix): rotating it would only chase that rounding down to the underflow range,
            // where the phase below loses its unit modulus
            const double g = hypot(gamma.x, gamma.y);
            const double shorter = alpha < beta ? alpha : beta, longer = alpha < beta ? beta : alpha;
            if (live && shorter > 1e-40 * longer && g > EPS * sqrt(alpha) * sqrt(beta)) {
                const Rotation rot = rotation_for(alpha, beta, gamma, g);
                for (int r = member; r < l; r += team) {
                    rotate(W[p * l + r], W[q * l + r], rot);
                    rotate(J[p * l + r], J[q * l + r], rot);
                }
                if (member == 0) rotated = 1;
            }
        }
        __syncthreads();
        if (!rotated) break;
    }
    __syncthreads();
    if (t == 0) *unconverged = rotated;     // still rotating after the last sweep allowed: the caller reports it
    for (int c = t; c < l; c += NT) {
        double s = 0.0;
        for (int r = 0; r < l; ++r) s += W[c * l + r].x * W[c * l + r].x + W[c * l + r].y * W[c * l + r].y;
        sigma[c] = sqrt(s);
    }
    __syncthreads();
    for (int c = t; c < l; c += NT) {
        int rank;
        QSV_JACOBI_RANK(rank, sigma, l, c);
        order[rank] = c;
    }
    __syncthreads();
    for (int e = t; e < l * l; e += NT) {
        const int rank = e / l, r = e % l, c = order[rank];
        Js[e] = J[c * l + r];
    }
}

// P = J^H J, column-major w x w (the identity up to the rounding the rotations accumulated)
__global__ __launch_bounds__(256) void k_site_small_gram(const amp_t *__restrict__ J, unsigned w, amp_t *__restrict__ P) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * w) return;
    const unsigned j = e / w, i = e % w;
    double re = 0.0, im = 0.0;
    for (unsigned r = 0; r < w; ++r) {
        const amp_t p = conj_mul(J[i * w + r], J[j * w + r]);
        re += p.x;
        im += p.y;
    }
    P[e] = amp_t{re, im};
}

// One Newton-Schulz step towards the nearest unitary matrix: out = (3 J - J P) / 2 with JP = J (J^H J).  A few hundred
// rotations per column leave J^H J - 1 at several 1e-15; the step takes it to the rounding of one product.
__global__ __launch_bounds__(256) void k_site_polish(const amp_t *__restrict__ J, const amp_t *__restrict__ JP, unsigned w,
                                                    amp_t *__restrict__ out) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * w) return;
    out[e] = amp_t{1.5 * J[e].x - 0.5 * JP[e].x, 1.5 * J[e].y - 0.5 * JP[e].y};
}

// S[j] = norm of column j of the column-major w x w matrix
__global__ __launch_bounds__(256) void k_site_column_norms(const amp_t *__restrict__ Wm, unsigned w, double *__restrict__ S) {
    const unsigned j = blockIdx.x * 256 + threadIdx.x;
    if (j >= w) return;
    double sum = 0.0;
    for (unsigned r = 0; r < w; ++r) sum += Wm[j * w + r].x * Wm[j * w + r].x + Wm[j * w + r].y * Wm[j * w + r].y;
    S[j] = sqrt(sum);
}

__global__ __launch_bounds__(256) void k_site_identity(amp_t *__restrict__ A, unsigned w) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e < w * w) A[e] = amp_t{e / w == e % w ? 1.0 : 0.0, 0.0};
}

// The scaling of one round from the sorted eigen-pairs (V column-major, lambda): VS = V diag(s), VI = V diag(1 / s), with
// s_j = 0 = 1 / s_j for a dropped direction.
__global__ __launch_bounds__(256) void k_site_scale(const amp_t *__restrict__ V, const double *__restrict__ lambda, unsigned w,
                                                   int round, double delta, amp_t *__restrict__ VS, amp_t *__restrict__ VI) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * w) return;
    const unsigned j = e / w;
    const double top = lambda[0], lam = lambda[j];
    double s = 0.0, inv = 0.0;
    if (top > 0.0) {
        if (round == 1) {
            s = sqrt(lam > delta * top ? lam : delta * top);
            inv = 1.0 / s;
        } else if (lam >= (round == 2 ? 4.0 * delta : 0.01) * top) {
            s = sqrt(lam);
            inv = 1.0 / s;
        }
    }
    const amp_t v = V[e];
    VS[e] = amp_t{v.x * s, v.y * s};
    VI[e] = amp_t{v.x * inv, v.y * inv};
}

// C = A . B, all column-major w x w; one thread per entry, the sum in index order
__global__ __launch_bounds__(256) void k_site_small_product(const amp_t *__restrict__ A, const amp_t *__restrict__ B, unsigned w,
                                                           amp_t *__restrict__ Cm) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * w) return;
    const unsigned j = e / w, r = e % w;
    double re = 0.0, im = 0.0;
    for (unsigned i = 0; i < w; ++i) {
        const amp_t p = plain_mul(A[i * w + r], B[j * w + i]);
        re += p.x;
        im += p.y;
    }
    Cm[e] = amp_t{re, im};
}

// The first k columns of the column-major T in the layout k_site_apply reads: (w x k) row-major for side 0, its
// conjugate transpose (k x w) row-major for side 1.
__global__ __launch_bounds__(256) void k_site_layout(const amp_t *__restrict__ T, unsigned w, unsigned k, int side,
                                                    amp_t *__restrict__ out) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * k) return;
    const unsigned j = e / w, c = e % w;
    const amp_t v = T[e];
    if (side == 0) out[c * k + j] = v;
    else out[e] = amp_t{v.x, -v.y};
}

// carry from the sorted rotated columns Ws (norm sigma_j): side 0 (k x w) carry[j, c] = conj(Ws[c, j]); side 1 (w x k)
// carry[c, j] = Ws[c, j]
__global__ __launch_bounds__(256) void k_site_carry(const amp_t *__restrict__ Ws, unsigned w, unsigned k, int side,
                                                   amp_t *__restrict__ carry) {
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    if (e >= w * k) return;
    const unsigned j = e / w, c = e % w;
    const amp_t v = Ws[e];
    if (side == 0) carry[e] = amp_t{v.x, -v.y};
    else carry[c * k + j] = v;
}

inline unsigned blocks256(uint64_t n) { return static_cast<unsigned>((n + 255) / 256); }

}  // namespace

int qsv_tensor_site_orthogonalise(int device, void *hip_stream, const void *dev_site, uint64_t L, uint64_t d, uint64_t R,
                                  int side, double rank_tol, void *dev_iso, void *dev_carry, uint64_t *rank,
                                  double *singular_values) {
    // every check before the first HIP call
    if (!dev_site || !dev_iso || !dev_carry || !rank) return qsv_fail(QSV_EINVAL, "null pointer");
    if (device < 0 || device >= 16) return qsv_fail(QSV_EINVAL, "device index out of range");
    if (side != 0 && side != 1) return qsv_fail(QSV_EINVAL, "side must be 0 (left) or 1 (right)");
    if (d < 2) return qsv_fail(QSV_EINVAL, "a site needs a grid of at least two points");
    if (L < 1 || R < 1) return qsv_fail(QSV_EINVAL, "empty bond");
    if (!(rank_tol >= 0.0) || !std::isfinite(rank_tol)) return qsv_fail(QSV_EINVAL, "rank_tol must be finite and >= 0");
    const uint64_t w = side == 0 ? R : L, other = side == 0 ? L : R;
    if (w > static_cast<uint64_t>(SITE_MAX_BOND))
        return qsv_fail(QSV_EINVAL, "bond " + std::to_string(w) + " exceeds QSV_SITE_MAX_BOND = " + std::to_string(SITE_MAX_BOND));
    if (d > (1ull << 31) || other > (1ull << 31) || d * other > (1ull << 36))
        return qsv_fail(QSV_EINVAL, "site too large for one call");
    const uint64_t N = d * other;

    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;

    const unsigned wu = static_cast<unsigned>(w), tiles = (wu + 15) / 16, wp = 16 * tiles;
    const uint64_t steps = (N + 15) / 16;
    const unsigned chunks = static_cast<unsigned>(steps / 4 < 1 ? 1 : steps / 4 > GRAM_MAX_CHUNKS ? GRAM_MAX_CHUNKS : steps / 4);
    const unsigned n_partials = 4 * chunks;
    const size_t big = sizeof(amp_t) * N * w, small = sizeof(amp_t) * w * w;
    const size_t bytes_partials = sizeof(amp_t) * n_partials * wp * wp;
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    DeviceBuffers buf;
    buf.reserve(*ctx, 2 * pad(big) + pad(bytes_partials) + 13 * pad(small) + pad(8 * w) + 256);
    amp_t *Q1, *Q2, *partials, *G, *Jw, *Gs, *V, *VS, *VI, *Wa, *Wb, *Tl, *Ws, *Wk, *Jr, *Pm;
    double *S;
    int *flags;       // one per Jacobi decomposition of the call
    if (!buf.alloc(&flags, 4 * sizeof(int)) || !buf.alloc(&Q1, big) || !buf.alloc(&Q2, big) || !buf.alloc(&partials, bytes_partials) || !buf.alloc(&G, small) ||
        !buf.alloc(&Jw, small) || !buf.alloc(&Gs, small) || !buf.alloc(&V, small) || !buf.alloc(&VS, small) ||
        !buf.alloc(&VI, small) || !buf.alloc(&Wa, small) || !buf.alloc(&Wb, small) || !buf.alloc(&Tl, small) ||
        !buf.alloc(&Ws, small) || !buf.alloc(&Wk, small) || !buf.alloc(&Jr, small) || !buf.alloc(&Pm, small) ||
        !buf.alloc(&S, 8 * w))
        return qsv_fail(QSV_ENOMEM, "site orthogonalisation workspace allocation failed");

    const double eps = 2.220446049250313e-16;
    const double root_n = std::sqrt(static_cast<double>(N));
    const double delta = 8.0 * eps * (static_cast<double>(w) > root_n ? static_cast<double>(w) : root_n);
    const unsigned small_blocks = blocks256(w * w);
    const dim3 gram_grid(tiles, (tiles + 3) / 4, chunks);
    auto gram = [&](const amp_t *X) {
        if (side == 0) hipLaunchKernelGGL(k_site_gram<0>, gram_grid, dim3(256), 0, stream, X, N, w, partials, wp);
        else hipLaunchKernelGGL(k_site_gram<1>, gram_grid, dim3(256), 0, stream, X, N, w, partials, wp);
        hipLaunchKernelGGL(k_site_gram_reduce, dim3(small_blocks), dim3(256), 0, stream, partials, n_partials, wu, wp,
                           side == 0 ? 1.0 : -1.0, G);
    };
    auto apply = [&](const amp_t *X, const amp_t *T, amp_t *out, uint64_t k) {
        const dim3 grid(static_cast<unsigned>((N + 127) / 128), static_cast<unsigned>((k + 63) / 64));
        if (side == 0) hipLaunchKernelGGL(k_site_apply<0>, grid, dim3(256), 0, stream, X, T, out, N, w, k);
        else hipLaunchKernelGGL(k_site_apply<1>, grid, dim3(256), 0, stream, X, T, out, N, w, k);
    };
    // A (kept intact) = sorted_cols . sorted_rot^H: the rotations of k_site_jacobi, polished towards unitarity, then the
    // rotated columns as one explicit product and their norms
    auto jacobi = [&](const amp_t *A, amp_t *sorted_cols, amp_t *sorted_rot, int slot) {
        hipLaunchKernelGGL(k_site_jacobi, dim3(1), dim3(JACOBI_THREADS), 0, stream, A, Wk, static_cast<int>(w), Jw, Jr,
                           flags + slot);
        hipLaunchKernelGGL(k_site_small_gram, dim3(small_blocks), dim3(256), 0, stream, Jr, wu, Pm);
        hipLaunchKernelGGL(k_site_small_product, dim3(small_blocks), dim3(256), 0, stream, Jr, Pm, wu, Wk);
        hipLaunchKernelGGL(k_site_polish, dim3(small_blocks), dim3(256), 0, stream, Jr, Wk, wu, sorted_rot);
        hipLaunchKernelGGL(k_site_small_product, dim3(small_blocks), dim3(256), 0, stream, A, sorted_rot, wu, sorted_cols);
        hipLaunchKernelGGL(k_site_column_norms, dim3(blocks256(w)), dim3(256), 0, stream, sorted_cols, wu, S);
    };

    std::vector<double> sv(w);
    uint64_t kept = 0;
    // everything queued on the stream; on failure the caller below still waits for it before the pool is handed on
    auto work = [&]() -> int {
    const amp_t *X = static_cast<const amp_t *>(dev_site);
    amp_t *w_now = Wa, *w_next = Wb;
    hipLaunchKernelGGL(k_site_identity, dim3(small_blocks), dim3(256), 0, stream, w_now, wu);
    for (int round = 1; round <= 3; ++round) {
        gram(X);
        jacobi(G, Gs, V, round - 1);
        hipLaunchKernelGGL(k_site_scale, dim3(small_blocks), dim3(256), 0, stream, V, S, wu, round, delta, VS, VI);
        hipLaunchKernelGGL(k_site_small_product, dim3(small_blocks), dim3(256), 0, stream, w_now, VS, wu, w_next);
        amp_t *swap = w_now;
        w_now = w_next;
        w_next = swap;
        if (round < 3) {
            amp_t *out = round == 1 ? Q1 : Q2;
            hipLaunchKernelGGL(k_site_layout, dim3(small_blocks), dim3(256), 0, stream, VI, wu, wu, side, Tl);
            apply(X, Tl, out, w);
            X = out;
        }
    }
    QSV_HIP(hipGetLastError());
    // singular value decomposition of the small factor: w_now J = U diag(sigma); V receives the sorted J
    jacobi(w_now, Ws, V, 3);
    int stuck[4] = {0, 0, 0, 0};
    QSV_HIP(hipMemcpyAsync(sv.data(), S, 8 * w, hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipMemcpyAsync(stuck, flags, sizeof(stuck), hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipStreamSynchronize(stream));
    if (stuck[0] || stuck[1] || stuck[2] || stuck[3])
        return qsv_fail(QSV_EHIP, "site orthogonalisation: the Jacobi sweeps did not converge");
    while (kept < w && sv[kept] > 0.0 && sv[kept] > rank_tol * sv[0]) ++kept;
    if (kept > N) kept = N;
    if (kept > 0) {
        const unsigned ku = static_cast<unsigned>(kept);
        hipLaunchKernelGGL(k_site_small_product, dim3(small_blocks), dim3(256), 0, stream, VI, V, wu, w_next);
        hipLaunchKernelGGL(k_site_layout, dim3(blocks256(w * kept)), dim3(256), 0, stream, w_next, wu, ku, side, Tl);
        apply(X, Tl, static_cast<amp_t *>(dev_iso), kept);
        hipLaunchKernelGGL(k_site_carry, dim3(blocks256(w * kept)), dim3(256), 0, stream, Ws, wu, ku, side,
                           static_cast<amp_t *>(dev_carry));
        QSV_HIP(hipGetLastError());
        QSV_HIP(hipStreamSynchronize(stream));      // the pool is free again only when the kernels are done
    }
    return QSV_OK;
    };
    const int status = work();
    if (status != QSV_OK) {
        (void)hipStreamSynchronize(stream);         // kernels may still be queued on the pool's memory
        return status;
    }
    if (singular_values) {
        const uint64_t count = N < w ? N : w;
        for (uint64_t i = 0; i < count; ++i) singular_values[i] = sv[i];
    }
    *rank = kept;
    return QSV_OK;
}

// Panel kernels of the randomized split: wide_panel_orthonormalise and factor_svd (for qsv_rsvd.hip).
//
// Fused tall-skinny kernels for the randomized split.  rocSOLVER's zgeqrf / zungqr / zgesvd on an (n x l) panel with
// l = k + 10 <= 64 columns are hundreds of microsecond-sized launches each (profiles/r01_mps_kernel_stats.csv: half of
// the GPU time of a split), and the range finder re-orthonormalises 15 times.  Any orthonormal basis of the same
// subspace gives the same U S Vh, so the panels are orthonormalised by shifted CholeskyQR3 (Fukaya et al., SIAM J.
// Sci. Comput. 42, 2020): three rounds of  G = Y^H Y,  R = chol(G + shift I),  Y <- Y R^-1 (a triangular solve per row)  -- three launches per
// round, every one a single pass over the panel; the shift of the first round makes the factorisation succeed for
// condition numbers up to 1/u, directions that are numerically absent are detected by their pivot in the later
// rounds and dropped (zero columns; Householder QR would invent arbitrary complements there).  The (l x m) projection
// B is never decomposed directly either: B^H is orthonormalised the same way (B^H = Qb Rb) and the l x l triangle Rb
// goes through a one-sided Jacobi SVD in a single workgroup (high relative accuracy, no bidiagonalisation).
#include <mutex>

#include "qsv_jacobi.h"
#include "qsv_linalg.h"

using namespace qsvl;
using namespace qsv_jacobi;

namespace {

constexpr int PANEL_ROWS = 64;      // rows per LDS tile
constexpr int PANEL_PITCH = PANEL_ROWS + 1;

// partials[block][i * l + j] = sum over the block's rows of conj(Y[r, i]) * Y[r, j]   (Y column-major, ld n)
// BANDS > 1: blockIdx.y takes one of BANDS slices of the entries (a short panel has too few row tiles to fill the chip,
// and one workgroup per tile spends 16 entries x 64 rows of dependent FMAs per thread)
template <int BANDS>
__global__ __launch_bounds__(256) void k_panel_gram(const amp_t *__restrict__ Y, uint64_t n, int l,
                                                   amp_t *__restrict__ partials, const int *__restrict__ settled) {
    if (settled && *settled) return;     // the previous round found the panel orthonormal already
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(smem_raw);   // [l][PANEL_PITCH]
    constexpr int PER_THREAD = LMAX * LMAX / 256 / BANDS;
    const int t = threadIdx.x + 256 * PER_THREAD * blockIdx.y, entries = l * l;
    amp_t acc[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) acc[k] = amp_t{0.0, 0.0};
    for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * PANEL_ROWS; r0 < n;
         r0 += static_cast<uint64_t>(gridDim.x) * PANEL_ROWS) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < l * PANEL_ROWS; idx += 256) {
            const int c = idx / PANEL_ROWS, r = idx % PANEL_ROWS;
            tile[c * PANEL_PITCH + r] = r0 + r < n ? Y[static_cast<uint64_t>(c) * n + r0 + r] : amp_t{0.0, 0.0};
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int e = t + 256 * k;
            if (e < entries) {
                const amp_t *ci = tile + (e / l) * PANEL_PITCH, *cj = tile + (e % l) * PANEL_PITCH;
                amp_t a = acc[k];
                for (int r = 0; r < PANEL_ROWS; ++r) {
                    const amp_t p = conj_mul(ci[r], cj[r]);
                    a.x += p.x;
                    a.y += p.y;
                }
                acc[k] = a;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int e = t + 256 * k;
        if (e < entries) partials[static_cast<size_t>(blockIdx.x) * entries + e] = acc[k];
    }
}

// partials[0][e] = partials[0][e] + partials[1][e] + ... in block order, one entry per thread with every load in flight:
// inside k_panel_factor (one workgroup, 128 registers per thread) that sum was a chain of load batches from another XCD's
// L2 -- 26 of the kernel's 80 us.
__global__ __launch_bounds__(256) void k_gram_reduce(amp_t *__restrict__ partials, int nblocks, int entries,
                                                    const int *__restrict__ skip) {
    if (skip && *skip) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    amp_t v[GRAM_BLOCKS];
#pragma unroll
    for (int b = 0; b < GRAM_BLOCKS; ++b)
        if (b < nblocks) v[b] = partials[static_cast<size_t>(b) * entries + e];
    amp_t s = {0.0, 0.0};
#pragma unroll
    for (int b = 0; b < GRAM_BLOCKS; ++b)
        if (b < nblocks) {
            s.x += v[b].x;
            s.y += v[b].y;
        }
    partials[e] = s;
}

// (1024 threads: the sum of the 64 partial Gram matrices is a chain of load batches per thread -- 16 entries x 2 batches
// with 256 threads, 130 us per launch on average and 29 % of the GPU time of the GKP Grover experiment; four times the
// threads quarter the chain, and the trailing updates of the factorisation shrink with it)
constexpr int FACTOR_THREADS = 1024;

// One workgroup: G = sum of the partials (+ shift), upper Cholesky factor R with G = R^H R, its inverse, and the running
// product r_total = R * r_prev.  first_round != 0 applies the CholeskyQR3 shift; otherwise pivots at rounding level
// mark absent directions: their column of R^-1 is zeroed (the panel column becomes zero).
__global__ __launch_bounds__(FACTOR_THREADS) void k_panel_factor(const amp_t *__restrict__ partials, int nblocks, int l,
                                                     uint64_t rows, int first_round,
                                                     const amp_t *__restrict__ r_prev, amp_t *__restrict__ r_total,
                                                     amp_t *__restrict__ r_out, const int *__restrict__ skip,
                                                     int *__restrict__ settled) {
    // `settled` (read by the NEXT round as its `skip`): set when this round's Gram matrix is the identity to 1e-7 -- after
    // this round's own normalisation the panel is orthonormal to rounding, so every kernel of the next round returns at once
    if (skip && *skip) {
        if (settled && threadIdx.x == 0) *settled = 1;
        return;
    }
    __shared__ amp_t G[LMAX * LMAX];
    __shared__ double deviation[FACTOR_THREADS / 64];
    __shared__ amp_t Stage[LMAX * LMAX];
    __shared__ double pivot_floor, shift;
    __shared__ int absent[LMAX];
    const int t = threadIdx.x, entries = l * l;
    for (int e = t; e < entries; e += FACTOR_THREADS) {
        amp_t s = {0.0, 0.0};
        int b = 0;
        for (; b + 16 <= nblocks; b += 16) {        // 16 independent loads in flight, summed in block order
            amp_t v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = partials[static_cast<size_t>(b + k) * entries + e];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                s.x += v[k].x;
                s.y += v[k].y;
            }
        }
        for (; b < nblocks; ++b) {
            const amp_t v = partials[static_cast<size_t>(b) * entries + e];
            s.x += v.x;
            s.y += v.y;
        }
        G[e] = s;
    }
    __syncthreads();
    if (t == 0) {
        double trace = 0.0, top = 0.0;
        for (int j = 0; j < l; ++j) {
            trace += G[j * l + j].x;
            top = fmax(top, G[j * l + j].x);
        }
        const double u = 1.1102230246251565e-16;
        shift = first_round ? 11.0 * (static_cast<double>(rows) * l + static_cast<double>(l) * (l + 1)) * u * trace : 0.0;
        pivot_floor = first_round ? 0.0 : static_cast<double>(l) * u * top;
    }
    if (settled) {
        double dev = first_round ? 1.0 : 0.0;      // the shifted round never settles anything
        for (int e = t; e < entries; e += FACTOR_THREADS) {
            const int i = e / l, k = e % l;
            if (k >= i) dev = fmax(dev, fmax(fabs(G[e].x - (i == k ? 1.0 : 0.0)), fabs(G[e].y)));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dev = fmax(dev, __shfl_xor(dev, o, 64));
        if ((t & 63) == 0) deviation[t >> 6] = dev;
    }
    __syncthreads();
    if (settled && t == 0) {
        double worst = 0.0;
        for (int w = 0; w < FACTOR_THREADS / 64; ++w) worst = fmax(worst, deviation[w]);
        *settled = worst < 1e-7;
    }
    // Blocked right-looking Cholesky, G = R^H R with R upper, 8 columns per step: the 8 x 8 diagonal block is factored by
    // the first wave alone (a wavefront executes its LDS instructions in order: no workgroup barriers inside), then all
    // threads solve the block row and update the trailing matrix -- 3 barriers per 8 columns instead of 3 per column.
    constexpr int NB = 8;
    for (int jb = 0; jb < l; jb += NB) {
        const int nb = l - jb < NB ? l - jb : NB;
        __syncthreads();
        if (t < 64) {
            // lane (i, k) = (t / 8, t % 8) keeps entry (i, k) of the block in a register; the pivot and the two factors of
            // every update come from the lanes of row p by wave shuffles -- the same operations on the same values as a
            // walk through LDS (which cost three LDS round trips per pivot: 3.2 us per block, a third of this kernel)
            const int i = t / NB, k = t % NB;
            const bool inside = i < nb && k < nb;
            amp_t g = inside ? G[(jb + i) * l + jb + k] : amp_t{0.0, 0.0};
            for (int p = 0; p < nb; ++p) {
                const double pivot = __shfl(g.x, p * NB + p, 64) + shift;
                const bool gone = !(pivot > pivot_floor);
                const double rjj = gone ? 1.0 : sqrt(pivot);
                if (i == p && k == p) g = amp_t{rjj, 0.0};
                else if (i == p && k > p && inside) g = gone ? amp_t{0.0, 0.0} : amp_t{g.x / rjj, g.y / rjj};   // the rest of row p
                if (t == 0) absent[jb + p] = gone;
                const amp_t ri = {__shfl(g.x, p * NB + i, 64), __shfl(g.y, p * NB + i, 64)};      // R[p][i]
                const amp_t rk = {__shfl(g.x, p * NB + k, 64), __shfl(g.y, p * NB + k, 64)};      // R[p][k]
                if (i > p && k >= i && inside) {     // the block's remaining entries (i, k), p < i <= k < nb
                    const amp_t pr = conj_mul(ri, rk);
                    g.x -= pr.x;
                    g.y -= pr.y;
                }
            }
            if (inside && k >= i) G[(jb + i) * l + jb + k] = g;
        }
        __syncthreads();
        // block row: R[jb + p][k] for k beyond the block, by forward substitution with the block's R^H
        for (int k = jb + nb + t; k < l; k += FACTOR_THREADS) {
            amp_t x[NB];
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                if (p < nb) {
                    amp_t acc = G[(jb + p) * l + k];
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        if (q < p) {
                            const amp_t pr = conj_mul(G[(jb + q) * l + jb + p], x[q]);
                            acc.x -= pr.x;
                            acc.y -= pr.y;
                        }
                    const double d = G[(jb + p) * l + jb + p].x;
                    x[p] = absent[jb + p] ? amp_t{0.0, 0.0} : amp_t{acc.x / d, acc.y / d};
                    G[(jb + p) * l + k] = x[p];
                } else {
                    x[p] = amp_t{0.0, 0.0};
                }
            }
        }
        __syncthreads();
        // trailing update G[i][k] -= sum_p conj(R[jb + p][i]) * R[jb + p][k] for jb + nb <= i <= k
        const int first = jb + nb, width = l - first;
        for (int e = t; e < width * width; e += FACTOR_THREADS) {
            const int i = first + e / width, k = first + e % width;
            if (k >= i) {
                amp_t acc = G[i * l + k];
#pragma unroll
                for (int p = 0; p < NB; ++p)
                    if (p < nb) {
                        const amp_t pr = conj_mul(G[(jb + p) * l + i], G[(jb + p) * l + k]);
                        acc.x -= pr.x;
                        acc.y -= pr.y;
                    }
                G[i * l + k] = acc;
            }
        }
    }
    __syncthreads();
    for (int e = t; e < entries; e += FACTOR_THREADS) {
        const int i = e / l, k = e % l;
        // the factor handed to k_panel_solve: upper triangle, diagonal 0 marks an absent direction
        r_out[e] = (k < i || absent[i]) ? amp_t{0.0, 0.0} : G[e];
        if (r_total) {
            amp_t sum = {0.0, 0.0};
            if (absent[i]) {
                // the panel column of an absent direction is zero: its row of the factor must not reach the SVD
            } else if (r_prev) {
                for (int q = i; q <= k; ++q) {   // both factors are upper triangular
                    const amp_t p = plain_mul(G[i * l + q], r_prev[q * l + k]);
                    sum.x += p.x;
                    sum.y += p.y;
                }
            } else if (k >= i) {
                sum = G[e];
            }
            Stage[e] = sum;   // staged: r_total may alias r_prev
        }
    }
    __syncthreads();
    if (r_total)
        for (int e = t; e < entries; e += FACTOR_THREADS) r_total[e] = Stage[e];
}

// Y <- Y R^-1 in place for the upper triangular R of k_panel_factor (row-major [i * l + j]): forward substitution per row,
// q_j = (y_j - sum_{i<j} q_i R[i][j]) / R[j][j], q_j = 0 for absent directions (R[j][j] == 0), in blocks of 8 columns.
// A workgroup stages 64 rows through LDS (coalesced both ways) together with a transposed copy of R; for every block the
// contribution of the columns solved so far is subtracted by all four waves (wave w takes two of the block's columns, so
// R[i][j] is an LDS broadcast), then the first wave finishes the 8 x 8 triangle for its 64 rows.
__global__ __launch_bounds__(256) void k_panel_solve(amp_t *__restrict__ Y, uint64_t n, int l,
                                                    const amp_t *__restrict__ R, const int *__restrict__ skip) {
    if (skip && *skip) return;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(smem_raw);   // [l][PANEL_PITCH]
    amp_t *Rs = tile + l * PANEL_PITCH;                  // [l][l], column-major copy: Rs[j * l + i] = R[i][j]
    constexpr int NB = 8;
    const int t = threadIdx.x, r = t & 63, wave = t >> 6;
    for (int e = t; e < l * l; e += 256) Rs[(e % l) * l + e / l] = R[e];
    for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * PANEL_ROWS; r0 < n;
         r0 += static_cast<uint64_t>(gridDim.x) * PANEL_ROWS) {
        const bool inside = r0 + r < n;
        __syncthreads();
        for (int c = wave; c < l; c += 4)
            tile[c * PANEL_PITCH + r] = inside ? Y[static_cast<uint64_t>(c) * n + r0 + r] : amp_t{0.0, 0.0};
        for (int jb = 0; jb < l; jb += NB) {
            const int nb = l - jb < NB ? l - jb : NB;
            __syncthreads();
            // subtract what the solved columns 0 .. jb-1 contribute to this block: wave w owns columns jb + 2w, jb + 2w + 1
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = 2 * wave + h;
                if (p < nb && jb > 0) {
                    const int j = jb + p;
                    const amp_t *col = Rs + j * l;
                    amp_t acc = tile[j * PANEL_PITCH + r];
                    int i = 0;
                    for (; i + 4 <= jb; i += 4) {
                        const amp_t p0 = plain_mul(tile[(i + 0) * PANEL_PITCH + r], col[i + 0]);
                        const amp_t p1 = plain_mul(tile[(i + 1) * PANEL_PITCH + r], col[i + 1]);
                        const amp_t p2 = plain_mul(tile[(i + 2) * PANEL_PITCH + r], col[i + 2]);
                        const amp_t p3 = plain_mul(tile[(i + 3) * PANEL_PITCH + r], col[i + 3]);
                        acc.x -= (p0.x + p1.x) + (p2.x + p3.x);
                        acc.y -= (p0.y + p1.y) + (p2.y + p3.y);
                    }
                    for (; i < jb; ++i) {
                        const amp_t pr = plain_mul(tile[i * PANEL_PITCH + r], col[i]);
                        acc.x -= pr.x;
                        acc.y -= pr.y;
                    }
                    tile[j * PANEL_PITCH + r] = acc;
                }
            }
            __syncthreads();
            if (wave == 0) {            // the block's own triangle, row by row of the tile: 28 products per row
                amp_t q[NB];
#pragma unroll
                for (int p = 0; p < NB; ++p) {
                    if (p < nb) {
                        const int j = jb + p;
                        const amp_t *col = Rs + j * l;
                        amp_t acc = tile[j * PANEL_PITCH + r];
#pragma unroll
                        for (int u = 0; u < NB; ++u)
                            if (u < p) {
                                const amp_t pr = plain_mul(q[u], col[jb + u]);
                                acc.x -= pr.x;
                                acc.y -= pr.y;
                            }
                        const double d = col[j].x;
                        q[p] = d != 0.0 ? amp_t{acc.x / d, acc.y / d} : amp_t{0.0, 0.0};
                        tile[j * PANEL_PITCH + r] = q[p];
                        if (inside) Y[static_cast<uint64_t>(j) * n + r0 + r] = q[p];
                    } else {
                        q[p] = amp_t{0.0, 0.0};
                    }
                }
            }
        }
    }
}

// SVD of the l x l matrix R (row-major) by one-sided Jacobi in one workgroup: R V = U S.  Column pairs follow a
// round-robin tournament (l/2 disjoint pairs per step, a few threads per pair); outputs are sorted by decreasing
// singular value: U, V column-major (l x l), S (l doubles).
// (Measured on the GKP Grover run, 64 x 64 factors: 830 us per launch with 256 threads -- 8 per column pair --, 800 with
// 512 and 1060 with 1024: the 63 workgroup barriers per sweep cost more with every wave added.  QSV_SVD_THREADS switches.)
constexpr int SVD_THREADS = 1024;     // launch bound; the launch uses split_options().svd_threads
__global__ __launch_bounds__(SVD_THREADS) void k_small_svd(const amp_t *__restrict__ R, int l, amp_t *__restrict__ U,
                                                  double *__restrict__ S, amp_t *__restrict__ V) {
    __shared__ amp_t W[LMAX * LMAX];    // working columns, column-major
    __shared__ amp_t Vw[LMAX * LMAX];
    __shared__ double sigma[LMAX];
    __shared__ int order[LMAX];
    __shared__ int rotated;
    const int t = threadIdx.x, NT = blockDim.x;
    for (int e = t; e < l * l; e += NT) {
        const int c = e / l, r = e % l;
        // the working matrix is R^H: its columns are the conjugated rows of the upper triangle, which the one-sided sweeps
        // orthogonalise in fewer passes than the columns of R itself (the triangle's rows are already nearly graded);
        // R^H = V S U^H, so the caller receives the factors with their roles exchanged
        const amp_t v = R[c * l + r];
        W[c * l + r] = amp_t{v.x, -v.y};
        Vw[c * l + r] = amp_t{r == c ? 1.0 : 0.0, 0.0};
    }
    const int lp = (l + 1) & ~1, pairs = lp / 2;
    int team = 1;                       // threads per pair: a power of two, pairs * team <= blockDim.x, team <= 64
    while (team * 2 * pairs <= NT && team < 64) team *= 2;
    const int pair = t / team, member = t % team;
    for (int sweep = 0; sweep < 40; ++sweep) {
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
            const double g2 = gamma.x * gamma.x + gamma.y * gamma.y;
            if (live && g2 > EPS * EPS * alpha * beta && g2 > 0.0) {
                const Rotation rot = rotation_for(alpha, beta, gamma, sqrt(g2));
                for (int r = member; r < l; r += team) {
                    rotate(W[p * l + r], W[q * l + r], rot);
                    rotate(Vw[p * l + r], Vw[q * l + r], rot);
                }
                if (member == 0) rotated = 1;
            }
        }
        __syncthreads();
        if (!rotated) break;
    }
    __syncthreads();
    for (int c = t; c < l; c += NT) {
        double s = 0.0;
        for (int r = 0; r < l; ++r) s += W[c * l + r].x * W[c * l + r].x + W[c * l + r].y * W[c * l + r].y;
        sigma[c] = sqrt(s);
    }
    __syncthreads();
    if (t == 0)                         // ranks by decreasing singular value (l <= 64)
        for (int c = 0; c < l; ++c) {
            int rank;
            QSV_JACOBI_RANK(rank, sigma, l, c);
            order[rank] = c;
        }
    __syncthreads();
    for (int e = t; e < l * l; e += NT) {
        const int rank = e / l, r = e % l, c = order[rank];
        const double s = sigma[c];
        const amp_t w = W[c * l + r];
        U[rank * l + r] = s > 0.0 ? amp_t{w.x / s, w.y / s} : amp_t{0.0, 0.0};
        V[rank * l + r] = Vw[c * l + r];
    }
    for (int rank = t; rank < l; rank += NT) S[rank] = sigma[order[rank]];
}

// ---- the same one-sided Jacobi SVD for factors wider than 64 columns (up to WIDE_FACTOR): the working matrices live in
// global memory (L2-resident) and every tournament step is one launch with a wave per column pair ------------------------
constexpr int WIDE_FACTOR = 256;

// W (column-major l x l) = R^H for the row-major upper triangular R; V = identity
__global__ __launch_bounds__(256) void k_jacobi_init(const amp_t *__restrict__ R, int l, amp_t *__restrict__ W,
                                                    amp_t *__restrict__ V) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < l * l; e += gridDim.x * 256) {
        const int c = e / l, r = e % l;
        const amp_t v = R[c * l + r];
        W[e] = amp_t{v.x, -v.y};
        V[e] = amp_t{r == c ? 1.0 : 0.0, 0.0};
    }
}

// one step of the round-robin tournament: block b rotates its pair of columns of W (and of V) if they are not orthogonal
__global__ __launch_bounds__(64) void k_jacobi_step(amp_t *__restrict__ W, amp_t *__restrict__ V, int l, int lp, int step,
                                                   int *__restrict__ rotated) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const ColumnPair cp = tournament_pair(lp, step, pair);
    const int p = cp.p, q = cp.q;
    if (q >= l) return;       // the padding column of an odd l sits out
    amp_t *wp = W + static_cast<size_t>(p) * l, *wq = W + static_cast<size_t>(q) * l;
    double alpha = 0.0, beta = 0.0;
    amp_t gamma = {0.0, 0.0};
    for (int r = lane; r < l; r += 64) {
        const amp_t x = wp[r], y = wq[r];
        QSV_JACOBI_ACCUMULATE(alpha, beta, gamma, x, y);
    }
    QSV_JACOBI_TEAM_REDUCE(alpha, beta, gamma, 64);
    const double g2 = gamma.x * gamma.x + gamma.y * gamma.y;
    if (!(g2 > EPS * EPS * alpha * beta) || !(g2 > 0.0)) return;
    const Rotation rot = rotation_for(alpha, beta, gamma, sqrt(g2));
    amp_t *vp = V + static_cast<size_t>(p) * l, *vq = V + static_cast<size_t>(q) * l;
    for (int r = lane; r < l; r += 64) {
        rotate(wp[r], wq[r], rot);
        rotate(vp[r], vq[r], rot);
    }
    if (lane == 0) *rotated = 1;
}

// singular values = column norms of W, sorted decreasingly; left = W / sigma, right = V in that order (column-major)
__global__ __launch_bounds__(256) void k_jacobi_finish(const amp_t *__restrict__ W, const amp_t *__restrict__ V, int l,
                                                      amp_t *__restrict__ left, double *__restrict__ S,
                                                      amp_t *__restrict__ right) {
    __shared__ double sigma[WIDE_FACTOR];
    __shared__ int order[WIDE_FACTOR];
    const int t = threadIdx.x;
    for (int c = t; c < l; c += 256) {
        double s = 0.0;
        for (int r = 0; r < l; ++r) {
            const amp_t w = W[static_cast<size_t>(c) * l + r];
            s += w.x * w.x + w.y * w.y;
        }
        sigma[c] = sqrt(s);
    }
    __syncthreads();
    for (int c = t; c < l; c += 256) {
        int rank;
        QSV_JACOBI_RANK(rank, sigma, l, c);
        order[rank] = c;
    }
    __syncthreads();
    for (int e = t; e < l * l; e += 256) {
        const int rank = e / l, r = e % l, c = order[rank];
        const double s = sigma[c];
        const amp_t w = W[static_cast<size_t>(c) * l + r];
        left[e] = s > 0.0 ? amp_t{w.x / s, w.y / s} : amp_t{0.0, 0.0};
        right[e] = V[static_cast<size_t>(c) * l + r];
    }
    for (int rank = t; rank < l; rank += 256) S[rank] = sigma[order[rank]];
}

}  // namespace

// (The kernels decompose R^H = V_r S U_r^H, hence the exchanged output arguments.)
int qsvl::factor_svd(hipStream_t stream, const amp_t *R, int l, amp_t *work, amp_t *Ur, double *S, amp_t *Vr, int *flag) {
    if (l <= LMAX) {
        hipLaunchKernelGGL(k_small_svd, dim3(1), dim3(qsv_split_rules::split_options().svd_threads), 0, stream, R, l, Vr, S, Ur);
        QSV_HIP(hipGetLastError());
        return QSV_OK;
    }
    // wider than the one-workgroup kernel: the same sweeps with the working matrices in global memory, one launch per
    // tournament step (rocSOLVER's zgesvd spends ~25 ms in bdsqr launch storms on a 110 x 110 factor)
    amp_t *W = work, *V = work + static_cast<size_t>(l) * l;
    hipLaunchKernelGGL(k_jacobi_init, dim3(64), dim3(256), 0, stream, R, l, W, V);
    const int lp = (l + 1) & ~1;
    for (int sweep = 0; sweep < 40; ++sweep) {
        QSV_HIP(hipMemsetAsync(flag, 0, sizeof(int), stream));
        for (int step = 0; step < lp - 1; ++step)
            hipLaunchKernelGGL(k_jacobi_step, dim3(lp / 2), dim3(64), 0, stream, W, V, l, lp, step, flag);
        int rotated = 0;
        QSV_HIP(hipMemcpyAsync(&rotated, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
        QSV_HIP(hipStreamSynchronize(stream));
        if (!rotated) break;
    }
    hipLaunchKernelGGL(k_jacobi_finish, dim3(1), dim3(256), 0, stream, W, V, l, Vr, S, Ur);
    QSV_HIP(hipGetLastError());
    return QSV_OK;
}

namespace {

// Shifted CholeskyQR3 of the column-major (n x l) panel Y, in place.  `r_total` (l x l, row-major, may be null) receives
// the triangular factor with  Y_in = Y_out * r_total.
// `rounds` = 2 for the intermediate panels of the power iteration: only their SPAN enters the next product, and after the
// shifted round and one plain round the basis is conditioned like O(1) (absent directions dropped) -- the third round,
// which takes the Gram matrix from ~1e-8 of the identity to rounding level, matters for the final Q and for Qb alone.
int panel_orthonormalise(hipStream_t stream, amp_t *Y, uint64_t n, int l, amp_t *partials, amp_t *r_factor,
                         amp_t *r_total, int *flags = nullptr, int rounds = 3) {
    const size_t lds = sizeof(amp_t) * l * PANEL_PITCH;
    static std::once_flag raised, raised_solve;     // attributes are process-wide: set once, whichever thread comes first
    static hipError_t raised_status = hipSuccess, raised_solve_status = hipSuccess;
    if (lds > 64 * 1024) {
        std::call_once(raised, [] {
            const int bytes = static_cast<int>(LMAX * PANEL_PITCH * sizeof(amp_t));
            raised_status = hipFuncSetAttribute(reinterpret_cast<const void *>(k_panel_gram<1>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (raised_status == hipSuccess)
                raised_status = hipFuncSetAttribute(reinterpret_cast<const void *>(k_panel_gram<4>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        });
        QSV_HIP(raised_status);
    }
    if (lds + sizeof(amp_t) * l * l > 64 * 1024) {
        std::call_once(raised_solve, [] {
            raised_solve_status = hipFuncSetAttribute(reinterpret_cast<const void *>(k_panel_solve),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      static_cast<int>((LMAX * PANEL_PITCH + LMAX * LMAX) * sizeof(amp_t)));
        });
        QSV_HIP(raised_solve_status);
    }
    const uint64_t tiles = (n + PANEL_ROWS - 1) / PANEL_ROWS;
    const int gram_blocks = static_cast<int>(tiles < GRAM_BLOCKS ? tiles : GRAM_BLOCKS);
    const unsigned apply_blocks = static_cast<unsigned>(tiles < 4096 ? tiles : 4096);
    for (int round = 0; round < rounds; ++round) {
        // flags[round] tells this round's kernels to return at once; the factor kernel of a round writes flags[round + 1]
        const int *skip = flags && round > 0 ? flags + round : nullptr;
        int *next = flags && round < 2 ? flags + round + 1 : nullptr;
        if (tiles <= 256) hipLaunchKernelGGL(k_panel_gram<4>, dim3(gram_blocks, 4), dim3(256), lds, stream, Y, n, l, partials, skip);
        else hipLaunchKernelGGL(k_panel_gram<1>, dim3(gram_blocks), dim3(256), lds, stream, Y, n, l, partials, skip);
        if (gram_blocks > 1)
            hipLaunchKernelGGL(k_gram_reduce, dim3((l * l + 255) / 256), dim3(256), 0, stream, partials, gram_blocks, l * l, skip);
        hipLaunchKernelGGL(k_panel_factor, dim3(1), dim3(FACTOR_THREADS), 0, stream, partials, 1, l, n, round == 0,
                           round == 0 ? nullptr : r_total, r_total, r_factor, skip, next);
        hipLaunchKernelGGL(k_panel_solve, dim3(apply_blocks), dim3(256), lds + sizeof(amp_t) * l * l, stream, Y, n, l,
                           r_factor, skip);
    }
    QSV_HIP(hipGetLastError());
    return QSV_OK;
}

// ---- panels wider than 64 columns: block Gram-Schmidt over 64-column blocks -------------------------------------------
// partials[block][i * lb + j] = sum over the block's rows of conj(Ya[r, i]) * Yb[r, j]  (two panels of la, lb <= 64 columns)
__global__ __launch_bounds__(256) void k_panel_cross(const amp_t *__restrict__ Ya, const amp_t *__restrict__ Yb,
                                                    uint64_t n, int la, int lb, amp_t *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    amp_t *ta = reinterpret_cast<amp_t *>(smem_raw);     // [la][PANEL_PITCH]
    amp_t *tb = ta + la * PANEL_PITCH;                   // [lb][PANEL_PITCH]
    const int t = threadIdx.x, entries = la * lb;
    amp_t acc[LMAX * LMAX / 256];
#pragma unroll
    for (int k = 0; k < LMAX * LMAX / 256; ++k) acc[k] = amp_t{0.0, 0.0};
    for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * PANEL_ROWS; r0 < n;
         r0 += static_cast<uint64_t>(gridDim.x) * PANEL_ROWS) {
        __syncthreads();
        for (int idx = t; idx < (la + lb) * PANEL_ROWS; idx += 256) {
            const int c = idx / PANEL_ROWS, r = idx % PANEL_ROWS;
            const amp_t *src = c < la ? Ya + static_cast<uint64_t>(c) * n : Yb + static_cast<uint64_t>(c - la) * n;
            ta[c * PANEL_PITCH + r] = r0 + r < n ? src[r0 + r] : amp_t{0.0, 0.0};
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LMAX * LMAX / 256; ++k) {
            const int e = t + 256 * k;
            if (e < entries) {
                const amp_t *ci = ta + (e / lb) * PANEL_PITCH, *cj = tb + (e % lb) * PANEL_PITCH;
                amp_t a = acc[k];
                for (int r = 0; r < PANEL_ROWS; ++r) {
                    const amp_t p = conj_mul(ci[r], cj[r]);
                    a.x += p.x;
                    a.y += p.y;
                }
                acc[k] = a;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LMAX * LMAX / 256; ++k) {
        const int e = t + 256 * k;
        if (e < entries) partials[static_cast<size_t>(blockIdx.x) * entries + e] = acc[k];
    }
}

// C (la x lb, row-major) = sum of the partials; optionally R[row0 + i][col0 + j] (+)= C[i][j] in the l x l factor
__global__ __launch_bounds__(256) void k_cross_reduce(const amp_t *__restrict__ partials, int nblocks, int la, int lb,
                                                     amp_t *__restrict__ C, amp_t *__restrict__ R, int l, int row0,
                                                     int col0, int accumulate) {
    const int entries = la * lb;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < entries; e += gridDim.x * 256) {
        amp_t s = {0.0, 0.0};
        for (int b = 0; b < nblocks; ++b) {
            const amp_t v = partials[static_cast<size_t>(b) * entries + e];
            s.x += v.x;
            s.y += v.y;
        }
        C[e] = s;
        if (R) {
            amp_t *dst = R + static_cast<size_t>(row0 + e / lb) * l + col0 + e % lb;
            *dst = accumulate ? amp_t{dst->x + s.x, dst->y + s.y} : s;
        }
    }
}

// Yb[r, j] -= sum_i Qa[r, i] * C[i][j]   (Qa: la columns, Yb: lb columns, C row-major la x lb)
__global__ __launch_bounds__(256) void k_panel_update(amp_t *__restrict__ Yb, const amp_t *__restrict__ Qa, uint64_t n,
                                                     int la, int lb, const amp_t *__restrict__ C) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(smem_raw);   // [la][PANEL_PITCH]
    amp_t *Cs = tile + la * PANEL_PITCH;                 // [la][lb]
    const int t = threadIdx.x, r = t % PANEL_ROWS, group = t / PANEL_ROWS;
    for (int e = t; e < la * lb; e += 256) Cs[e] = C[e];
    for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * PANEL_ROWS; r0 < n;
         r0 += static_cast<uint64_t>(gridDim.x) * PANEL_ROWS) {
        __syncthreads();
        for (int idx = t; idx < la * PANEL_ROWS; idx += 256) {
            const int c = idx / PANEL_ROWS, rr = idx % PANEL_ROWS;
            tile[c * PANEL_PITCH + rr] = r0 + rr < n ? Qa[static_cast<uint64_t>(c) * n + r0 + rr] : amp_t{0.0, 0.0};
        }
        __syncthreads();
        if (r0 + r < n)
            for (int j = group; j < lb; j += 256 / PANEL_ROWS) {
                amp_t acc = Yb[static_cast<uint64_t>(j) * n + r0 + r];
                for (int i = 0; i < la; ++i) {
                    const amp_t p = plain_mul(tile[i * PANEL_PITCH + r], Cs[i * lb + j]);
                    acc.x -= p.x;
                    acc.y -= p.y;
                }
                Yb[static_cast<uint64_t>(j) * n + r0 + r] = acc;
            }
    }
}

// out[row0 + i][col0 + j] = src[i][j] for an (h x w) row-major block `src` inside the l x l row-major `out`
__global__ __launch_bounds__(256) void k_place_block(amp_t *__restrict__ out, int l, int row0, int col0,
                                                    const amp_t *__restrict__ src, int h, int w) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < h * w; e += gridDim.x * 256)
        out[static_cast<size_t>(row0 + e / w) * l + col0 + e % w] = src[e];
}

}  // namespace

// Shifted CholeskyQR3 on 64-column blocks, each first projected twice against the blocks before it (block classical
// Gram-Schmidt with re-orthogonalisation); r_total comes out block upper triangular.
int qsvl::wide_panel_orthonormalise(hipStream_t stream, amp_t *Y, uint64_t n, int l, amp_t *partials, amp_t *scratch,
                                    amp_t *r_total, int *flags, int rounds) {
    if (l <= LMAX) return panel_orthonormalise(stream, Y, n, l, partials, scratch, r_total, flags, rounds);
    static std::once_flag raised;
    static hipError_t raised_status = hipSuccess;
    std::call_once(raised, [] {
        const int big = static_cast<int>((2 * LMAX * PANEL_PITCH) * sizeof(amp_t));
        raised_status = hipFuncSetAttribute(reinterpret_cast<const void *>(k_panel_cross),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, big);
        if (raised_status == hipSuccess)
            raised_status = hipFuncSetAttribute(reinterpret_cast<const void *>(k_panel_update),
                                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                                static_cast<int>((LMAX * PANEL_PITCH + LMAX * LMAX) * sizeof(amp_t)));
    });
    QSV_HIP(raised_status);
    amp_t *block_factor = scratch, *cross = scratch + LMAX * LMAX;
    const uint64_t tiles = (n + PANEL_ROWS - 1) / PANEL_ROWS;
    const int red_blocks = static_cast<int>(tiles < GRAM_BLOCKS ? tiles : GRAM_BLOCKS);
    const unsigned row_blocks = static_cast<unsigned>(tiles < 4096 ? tiles : 4096);
    if (r_total) QSV_HIP(hipMemsetAsync(r_total, 0, sizeof(amp_t) * l * l, stream));
    for (int c0 = 0; c0 < l; c0 += LMAX) {
        const int w = l - c0 < LMAX ? l - c0 : LMAX;
        amp_t *Yj = Y + static_cast<uint64_t>(c0) * n;
        for (int pass = 0; pass < 2 && c0 > 0; ++pass)
            for (int p0 = 0; p0 < c0; p0 += LMAX) {
                const amp_t *Qi = Y + static_cast<uint64_t>(p0) * n;        // earlier blocks are full 64-column blocks
                hipLaunchKernelGGL(k_panel_cross, dim3(red_blocks), dim3(256), sizeof(amp_t) * (LMAX + w) * PANEL_PITCH,
                                   stream, Qi, Yj, n, LMAX, w, partials);
                hipLaunchKernelGGL(k_cross_reduce, dim3(4), dim3(256), 0, stream, partials, red_blocks, LMAX, w, cross,
                                   r_total, l, p0, c0, 1);
                hipLaunchKernelGGL(k_panel_update, dim3(row_blocks), dim3(256),
                                   sizeof(amp_t) * (LMAX * PANEL_PITCH + LMAX * w), stream, Yj, Qi, n, LMAX, w, cross);
            }
        // the block itself; its triangular factor goes on the diagonal of r_total
        amp_t *diag = r_total ? cross : nullptr;       // w x w, row-major, reuses the cross buffer
        const int rc = panel_orthonormalise(stream, Yj, n, w, partials, block_factor, diag, flags, rounds);
        if (rc) return rc;
        if (r_total) hipLaunchKernelGGL(k_place_block, dim3(4), dim3(256), 0, stream, r_total, l, c0, c0, diag, w, w);
    }
    QSV_HIP(hipGetLastError());
    return QSV_OK;
}

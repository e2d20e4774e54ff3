// The exact split of a matrix-product-state update: tensor_svd (cv_simulator/mps.py:52-97) on the GPU.
//
//   qsvg_svd_split   verified low-rank route (qsv_rsvd.hip) -> rocSOLVER zgesdd (guarded) -> one-sided Jacobi sweeps over
//                    the whole matrix, seeded by zgesdd (jacobi_full_split) -> rocSOLVER zgesvd
// (The randomized branch is qsv_rsvd.hip; the host-side rules of both are in qsv_split_rules.h.)
#include <algorithm>
#include <cstdio>
#include <vector>

#include "qsv_jacobi.h"
#include "qsv_linalg.h"

using namespace qsvl;
using namespace qsv_jacobi;
using namespace qsv_split_rules;

namespace {

// m1[row, i] = sqrt(s_i) * vt[row * k + i]  (i < r): compacts the (rows x k) factor to (rows x r)
__global__ __launch_bounds__(QSV_BLOCK) void k_scale_columns(const amp_t *__restrict__ vt, amp_t *__restrict__ m1,
                                                            uint64_t rows, uint64_t k, uint64_t r,
                                                            const double *__restrict__ s) {
    const uint64_t total = rows * r;
    for (uint64_t o = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t row = o / r, i = o % r;
        const double w = sqrt(s[i]);
        const amp_t v = vt[row * k + i];
        m1[o] = amp_t{w * v.x, w * v.y};
    }
}

// m2[i, c] = sqrt(s_i) * u[i * cols + c]  (i < r)
__global__ __launch_bounds__(QSV_BLOCK) void k_scale_rows(const amp_t *__restrict__ u, amp_t *__restrict__ m2,
                                                         uint64_t cols, uint64_t r, const double *__restrict__ s) {
    const uint64_t total = r * cols;
    for (uint64_t o = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const double w = sqrt(s[o / cols]);
        const amp_t v = u[o];
        m2[o] = amp_t{w * v.x, w * v.y};
    }
}

// ---- one-sided Jacobi SVD of a whole matrix: the exact split of a theta that is NOT numerically low-rank ---------------
// X (column-major L x k, k <= L, k <= JACOBI_MAX_COLUMNS) holds the k shorter vectors of theta; X J = Q S with J unitary
// (k x k) and orthogonal columns Q S.  A workgroup per column pair and launch per tournament step, as the wide factor above,
// but with 256 threads per pair (columns are thousands of entries long) -- rocSOLVER's zgesvd needs 1.35 s for a
// 1200 x 1200 matrix of rank 700 and 5 s at 2000 x 2000 (bdsqr launch storms); these sweeps take a fifth of that.
// squared norms of the k columns of an L x k matrix, element (r, c) at src[r * stride_row + c * stride_col]
__global__ __launch_bounds__(256) void k_column_norms(const amp_t *__restrict__ src, uint64_t stride_row, uint64_t stride_col,
                                                     uint64_t L, double *__restrict__ norms) {
    __shared__ double red[4];
    const amp_t *col = src + static_cast<uint64_t>(blockIdx.x) * stride_col;
    double s = 0.0;
    for (uint64_t r = threadIdx.x; r < L; r += 256) {
        const amp_t v = col[r * stride_row];
        s += v.x * v.x + v.y * v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) norms[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// W[:, c] = source column order[c]; the source is either column-major (L x k: stride_row = 1, stride_col = L) or the
// row-major (L x k) matrix (stride_row = k, stride_col = 1).  J = that permutation, so that X J = W holds for the source X.
__global__ __launch_bounds__(256) void k_jacobi_gather(const amp_t *__restrict__ src, uint64_t stride_row, uint64_t stride_col,
                                                      const int *__restrict__ order, amp_t *__restrict__ W,
                                                      amp_t *__restrict__ J, uint64_t L, int k) {
    const uint64_t total = L * static_cast<uint64_t>(k);
    for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < total; o += gridDim.x * 256ull) {
        const uint64_t r = o % L, c = o / L;
        W[o] = src[r * stride_row + static_cast<uint64_t>(order[c]) * stride_col];
    }
    const uint64_t kk = static_cast<uint64_t>(k) * k;
    for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < kk; o += gridDim.x * 256ull)
        J[o] = amp_t{static_cast<int>(o % k) == order[o / k] ? 1.0 : 0.0, 0.0};      // column-major: row o % k, column o / k
}

// J (column-major k x k) = the conjugate transpose of the column-major k x k matrix `vh`
__global__ __launch_bounds__(256) void k_jacobi_seed(const amp_t *__restrict__ vh, amp_t *__restrict__ J, int k) {
    const uint64_t kk = static_cast<uint64_t>(k) * k;
    for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < kk; o += gridDim.x * 256ull) {
        const uint64_t i = o % k, c = o / k;
        const amp_t v = vh[c + i * k];
        J[o] = amp_t{v.x, -v.y};
    }
}

// `floor2`: squared norm below which a column counts as numerically zero (see jacobi_full_split) and sits out
__global__ __launch_bounds__(256) void k_jacobi_pair(amp_t *__restrict__ W, amp_t *__restrict__ J, uint64_t L, int k, int kp,
                                                    int step, double floor2, int *__restrict__ rotated) {
    __shared__ double red[4][4];
    const int pair = blockIdx.x, t = threadIdx.x;
    const ColumnPair cp = tournament_pair(kp, step, pair);
    const int p = cp.p, q = cp.q;
    if (q >= k) return;       // the padding column of an odd k sits out
    amp_t *wp = W + static_cast<uint64_t>(p) * L, *wq = W + static_cast<uint64_t>(q) * L;
    double alpha = 0.0, beta = 0.0;
    amp_t gamma = {0.0, 0.0};
    for (uint64_t r = t; r < L; r += 256) {
        const amp_t x = wp[r], y = wq[r];
        QSV_JACOBI_ACCUMULATE(alpha, beta, gamma, x, y);
    }
    QSV_JACOBI_TEAM_REDUCE(alpha, beta, gamma, 64);
    if ((t & 63) == 0) {
        red[t >> 6][0] = alpha;
        red[t >> 6][1] = beta;
        red[t >> 6][2] = gamma.x;
        red[t >> 6][3] = gamma.y;
    }
    __syncthreads();
    alpha = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    beta = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    gamma.x = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    gamma.y = (red[0][3] + red[1][3]) + (red[2][3] + red[3][3]);
    // orthogonal to the rounding level of an L-term inner product, sqrt(L) eps (LAPACK's zgesvj uses the same tolerance):
    // below it the computed gamma is noise and the sweeps would never end
    const double g2 = gamma.x * gamma.x + gamma.y * gamma.y;
    if (!(g2 > static_cast<double>(L) * EPS * EPS * alpha * beta) || !(g2 > 0.0)) return;      // every thread holds the same sums
    if (!(alpha > floor2) || !(beta > floor2)) return;
    const Rotation rot = rotation_for(alpha, beta, gamma, sqrt(g2));
    for (uint64_t r = t; r < L; r += 256) rotate(wp[r], wq[r], rot);
    amp_t *jp = J + static_cast<uint64_t>(p) * k, *jq = J + static_cast<uint64_t>(q) * k;
    for (int r = t; r < k; r += 256) rotate(jp[r], jq[r], rot);
    if (t == 0) *rotated = 1;
}

// The two factors of the split from the converged sweeps: `order[a]` = working column of the a-th largest value,
// sigma2 = squared column norms.  long_side[x, a] = W[x, order[a]] / sigma_a^(1/2) (the unit vector times sqrt(sigma)),
// short_side[i, a] = J[i, order[a]] * sigma_a^(1/2), either side conjugated on request.  Both are written into row-major
// (rows x r) / (r x cols) outputs through (stride_x, stride_a).
__global__ __launch_bounds__(256) void k_jacobi_factors(const amp_t *__restrict__ W, const amp_t *__restrict__ J,
                                                       const int *__restrict__ order, const double *__restrict__ sigma2,
                                                       uint64_t L, int k, uint64_t r, amp_t *__restrict__ long_out,
                                                       uint64_t long_sx, uint64_t long_sa, amp_t *__restrict__ short_out,
                                                       uint64_t short_si, uint64_t short_sa, int conj_long, int conj_short) {
    const uint64_t n_long = L * r, n_short = static_cast<uint64_t>(k) * r;
    for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < n_long + n_short; o += gridDim.x * 256ull) {
        if (o < n_long) {
            const uint64_t x = o % L, a = o / L;
            const int c = order[a];
            const double sigma = sqrt(sigma2[c]), w = sigma > 0.0 ? 1.0 / sqrt(sigma) : 0.0;
            const amp_t v = W[static_cast<uint64_t>(c) * L + x];
            long_out[x * long_sx + a * long_sa] = amp_t{v.x * w, conj_long ? -v.y * w : v.y * w};
        } else {
            const uint64_t e = o - n_long, i = e % k, a = e / k;
            const int c = order[a];
            const double w = sqrt(sqrt(sigma2[c]));
            const amp_t v = J[static_cast<uint64_t>(c) * k + i];
            short_out[i * short_si + a * short_sa] = amp_t{v.x * w, conj_short ? -v.y * w : v.y * w};
        }
    }
}

// The exact split by one-sided Jacobi sweeps over the whole matrix (k_jacobi_pair): theta is left untouched;
// QSV_UNDECIDED when the matrix is outside what the sweeps take or they did not converge (the library SVD decides then).
//
// Started from the columns themselves the sweeps crawl on graded matrices (25 sweeps at 120 x 120 with singular values over
// six decades, 40+ at 1200 x 1200).  `seed_u` / `seed_vh` != null: the factors of rocSOLVER's zgesdd of theta^T (column-major
// cols x k and k x rows) -- through the eigenvectors of A^H A, good to ~1e-8 sigma_max, useless as an answer under a tight
// tolerance but an excellent preconditioner: X J0 with J0 the seed's unitary factor has nearly orthogonal columns, and the
// sweeps only polish (X J = W holds to rounding whatever the seed is, because W is recomputed as the product).
int jacobi_full_split(RocblasApi &a, rocblas_handle h, hipStream_t stream, const amp_t *theta, uint64_t rows, uint64_t cols,
                      int64_t max_bond_dim, double abs_err, double rel_err, amp_t *m1, amp_t *m2, uint64_t capacity,
                      uint64_t *rank_out, double *s_host, DeviceBuffers &buf, const amp_t *seed_u, const amp_t *seed_vh) {
    const bool wide = rows <= cols;          // the k shorter vectors: rows of theta (contiguous) or its columns
    const uint64_t k64 = wide ? rows : cols, L = wide ? cols : rows;
    if (k64 < 2 || k64 > static_cast<uint64_t>(JACOBI_MAX_COLUMNS)) return QSV_UNDECIDED;
    const int k = static_cast<int>(k64), kp = (k + 1) & ~1;
    const bool seeded = seed_u && seed_vh && a.zgemm;
    amp_t *W = nullptr, *J = nullptr;      // from the caller's workspace (its reservation counts them in)
    double *norms = nullptr;
    int *order = nullptr, *flag = nullptr;
    if (!buf.alloc(&W, sizeof(amp_t) * L * k64) || !buf.alloc(&J, sizeof(amp_t) * k64 * k64) ||
        !buf.alloc(&norms, sizeof(double) * k64) || !buf.alloc(&order, sizeof(int) * k64) || !buf.alloc(&flag, sizeof(int)))
        return QSV_UNDECIDED;
    std::vector<double> host_norms(k);
    std::vector<int> host_order(k);
    auto sorted_by_norm = [&]() -> int {      // host_order[a] = column with the a-th largest norm
        QSV_HIP(hipMemcpyAsync(host_norms.data(), norms, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
        QSV_HIP(hipStreamSynchronize(stream));
        for (int c = 0; c < k; ++c) host_order[c] = c;
        std::stable_sort(host_order.begin(), host_order.end(), [&](int x, int y) { return host_norms[x] > host_norms[y]; });
        QSV_HIP(hipMemcpyAsync(order, host_order.data(), sizeof(int) * k, hipMemcpyHostToDevice, stream));
        QSV_HIP(hipStreamSynchronize(stream));    // host_order is reused
        return QSV_OK;
    };
    // The working matrix: X (L x k) with X[x, c] = theta[c, x] (wide) or theta[x, c] (tall) -- or, seeded and tall, conj(X),
    // whose product with the seed is a plain library GEMM (M = theta^T is what the buffer holds column-major):
    //   wide:  M = U' S V'^H  ->  X = M,          J0 = V' = (seed_vh)^H,  W = M (seed_vh)^H
    //   tall:  M^H = V' S U'^H ->  conj(X) = M^H,  J0 = U' = seed_u,       W = M^H seed_u
    const bool conj_work = seeded && !wide;
    int rc;
    if (seeded) {
        const rocblas_int Li = static_cast<rocblas_int>(L);
        const rocblas_operation N = rocblas_operation_none, Cc = rocblas_operation_conjugate_transpose;
        bool ok;
        if (wide) {
            hipLaunchKernelGGL(k_jacobi_seed, dim3(1024), dim3(256), 0, stream, seed_vh, J, k);
            ok = zgemm(a, h, N, Cc, Li, k, k, theta, Li, seed_vh, k, W, Li);
        } else {
            QSV_HIP(hipMemcpyAsync(J, seed_u, sizeof(amp_t) * k64 * k64, hipMemcpyDeviceToDevice, stream));
            ok = zgemm(a, h, Cc, N, Li, k, k, theta, k, seed_u, k, W, Li);
        }
        if (!ok) return QSV_UNDECIDED;
        QSV_HIP(hipGetLastError());
    } else {
        // element (x, c) of X: wide theta -> theta[c, x] (buffer read column-major with ld cols); tall theta -> theta[x, c];
        // columns in decreasing norm first (de Rijk)
        const uint64_t stride_row = wide ? 1 : cols, stride_col = wide ? cols : 1;
        hipLaunchKernelGGL(k_column_norms, dim3(k), dim3(256), 0, stream, theta, stride_row, stride_col, L, norms);
        QSV_HIP(hipGetLastError());
        rc = sorted_by_norm();
        if (rc) return rc;
        hipLaunchKernelGGL(k_jacobi_gather, dim3(1024), dim3(256), 0, stream, theta, stride_row, stride_col, order, W, J, L, k);
    }
    // Columns below the dust floor (dust_floor2): their singular values are numerically zero -- LAPACK returns noise of that
    // size for them too -- and mutually orthogonal dust is not worth sweeps that never end (rotations among the large columns
    // keep re-randomising it).  X = W J^H holds whether or not they are orthogonal, so the product of the two factors is unaffected.
    hipLaunchKernelGGL(k_column_norms, dim3(k), dim3(256), 0, stream, W, static_cast<uint64_t>(1), L, L, norms);
    QSV_HIP(hipGetLastError());
    QSV_HIP(hipMemcpyAsync(host_norms.data(), norms, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipStreamSynchronize(stream));
    double frobenius2 = 0.0;
    for (double v : host_norms) frobenius2 += v;
    const double floor2 = dust_floor2(L, frobenius2);
    bool converged = false;
    const int max_sweeps = seeded ? 24 : 40;       // a seeded run that needs more is not being helped by its seed
    int sweeps = 0;
    for (; sweeps < max_sweeps && !converged; ++sweeps) {
        QSV_HIP(hipMemsetAsync(flag, 0, sizeof(int), stream));
        for (int step = 0; step < kp - 1; ++step)
            hipLaunchKernelGGL(k_jacobi_pair, dim3(kp / 2), dim3(256), 0, stream, W, J, L, k, kp, step, floor2, flag);
        QSV_HIP(hipGetLastError());
        int rotated = 0;
        QSV_HIP(hipMemcpyAsync(&rotated, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
        QSV_HIP(hipStreamSynchronize(stream));
        converged = !rotated;
    }
    if (split_options().trace)
        fprintf(stderr, "[qsv split] %llu x %llu: %sJacobi sweeps over the whole matrix: %d%s\n",
                static_cast<unsigned long long>(rows), static_cast<unsigned long long>(cols), seeded ? "seeded " : "", sweeps,
                converged ? "" : " (not converged)");
    if (!converged) return QSV_UNDECIDED;
    hipLaunchKernelGGL(k_column_norms, dim3(k), dim3(256), 0, stream, W, static_cast<uint64_t>(1), L, L, norms);
    QSV_HIP(hipGetLastError());
    rc = sorted_by_norm();
    if (rc) return rc;
    // (dust is relabelled -- values_from_norms --: if the rule keeps such a column anyway (rel_err = abs_err = 0) its outer
    // product W[:, c] J[:, c]^H enters the factors unchanged -- sigma only decides how the two factors share it)
    std::vector<double> sorted2(k);
    for (int c = 0; c < k; ++c) sorted2[c] = host_norms[host_order[c]];
    bool relabelled = false;
    const std::vector<double> sv = values_from_norms(sorted2, floor2, &relabelled);
    if (relabelled) {
        for (int c = 0; c < k; ++c) host_norms[host_order[c]] = sorted2[c];
        QSV_HIP(hipMemcpyAsync(norms, host_norms.data(), sizeof(double) * k, hipMemcpyHostToDevice, stream));
        QSV_HIP(hipStreamSynchronize(stream));
    }
    const uint64_t r = kept_rank(sv, max_bond_dim, abs_err, rel_err);
    if (r > capacity) return qsv_fail(QSV_EINVAL, "output buffers are smaller than the kept bond dimension");
    if (r > 0) {
        // X = W J^H (or its conjugate).  wide: theta = X^T: m2 (r x cols) takes the long vectors, m1 (rows x r) the rotations;
        // tall: theta = X: the other way round
        amp_t *long_out = wide ? m2 : m1, *short_out = wide ? m1 : m2;
        const uint64_t long_sx = wide ? 1 : r, long_sa = wide ? cols : 1, short_si = wide ? r : 1, short_sa = wide ? 1 : cols;
        hipLaunchKernelGGL(k_jacobi_factors, dim3(1024), dim3(256), 0, stream, W, J, order, norms, L, k, r, long_out, long_sx,
                           long_sa, short_out, short_si, short_sa, conj_work ? 1 : 0, conj_work ? 0 : 1);
        QSV_HIP(hipGetLastError());
    }
    QSV_HIP(hipStreamSynchronize(stream));   // the workspace is freed on return
    if (s_host)
        for (int c = 0; c < k; ++c) s_host[c] = sv[c];
    *rank_out = r;
    return QSV_OK;
}

}  // namespace

// tensor_svd (cv_simulator/mps.py:52-97) of a row-major (rows x cols) device matrix:
//   theta = U S Vh,  r from the truncation rule,  m1 = U[:, :r] sqrt(S[:r]),  m2 = sqrt(S[:r]) Vh[:r, :].
// rocSOLVER is column-major, so it factors theta^T = U' S V'^H (cols x rows); then U = (V'^H)^T and Vh = U'^T, i.e.
// the column-major U' buffer is the row-major Vh and the column-major V'^H buffer is the row-major U: no transposes.
int qsvg_svd_split(int device, hipStream_t stream, amp_t *theta, uint64_t rows, uint64_t cols, int64_t max_bond_dim,
                   double abs_err, double rel_err, amp_t *m1, amp_t *m2, uint64_t capacity, uint64_t *rank_out,
                   double *s_host) {
    const uint64_t lim = 0x7fffffffull;
    if (rows > lim || cols > lim) return qsv_fail(QSV_EINVAL, "matrix dimension exceeds 2^31 - 1");
    RocblasApi &a = api();
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;
    rocblas_handle h = handle_of(*ctx, &rc);
    if (!h) return rc;
    if (!a.zgesvd) return qsv_fail(QSV_EHIP, "rocSOLVER could not be loaded (librocsolver.so.0): no SVD available");
    const uint64_t k = rows < cols ? rows : cols;
    const SplitOptions &opt = split_options();
    double frobenius_squared = -1.0;      // filled in by the verified route when it gets far enough to measure it
    if (opt.shortcuts && opt.fused_panels) {     // any tolerance: the route verifies itself (or declines)
        const int fast = try_verified_low_rank(a, h, *ctx, theta, rows, cols, max_bond_dim, abs_err, rel_err, m1, m2, capacity,
                                               rank_out, s_host, k, &frobenius_squared);
        if (fast != QSV_UNDECIDED) return fast;
    }
    DeviceBuffers buf;
    buf.reserve(*ctx, sizeof(amp_t) * (cols * k + k * rows + 2 * rows * cols + k * k) + 32 * k + 16384);   // + the Jacobi route's copy
    double *dS = nullptr, *dE = nullptr;
    amp_t *dU = nullptr, *dV = nullptr;
    rocblas_int *dinfo = nullptr;
    if (!buf.alloc(&dS, sizeof(double) * k) || !buf.alloc(&dE, sizeof(double) * k) ||
        !buf.alloc(&dU, sizeof(amp_t) * cols * k) || !buf.alloc(&dV, sizeof(amp_t) * k * rows) ||
        !buf.alloc(&dinfo, sizeof(rocblas_int)))
        return qsv_fail(QSV_ENOMEM, "device allocation of the SVD factors failed");
    std::vector<double> sv(k);
    rocblas_int info = 0;
    const rocblas_int ci = static_cast<rocblas_int>(cols), ri = static_cast<rocblas_int>(rows), ki = static_cast<rocblas_int>(k);
    auto fetch_values = [&]() -> int {
        QSV_HIP(hipMemcpyAsync(sv.data(), dS, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
        QSV_HIP(hipMemcpyAsync(&info, dinfo, sizeof(info), hipMemcpyDeviceToHost, stream));
        QSV_HIP(hipStreamSynchronize(stream));
        return QSV_OK;
    };
    // rocSOLVER's zgesvd needs seconds on the graded spectra of these matrices (5 s at 2000 x 2000); its zgesdd takes 0.17 s
    // and is used when the truncation cannot notice its floor (gram_values_decide); otherwise theta is restored, and
    // zgesdd's factors seed the Jacobi sweeps where those fit (exact_route)
    bool decided = false;
    const ExactRoute route = exact_route(rows, cols, abs_err, rel_err, frobenius_squared, opt);
    const bool loose = route.loose, jacobi_fits = route.jacobi_fits;
    bool have_seed = false;
    if (a.zgesdd && opt.shortcuts && (loose || jacobi_fits)) {
        amp_t *backup = nullptr;
        if (buf.alloc(&backup, sizeof(amp_t) * rows * cols)) {
            QSV_HIP(hipMemcpyAsync(backup, theta, sizeof(amp_t) * rows * cols, hipMemcpyDeviceToDevice, stream));
            if (a.zgesdd(h, rocblas_svect_singular, rocblas_svect_singular, ci, ri, Z(theta), ci, dS, Z(dU), ci, Z(dV), ki,
                         dinfo) == rocblas_status_success) {
                const int rc_fetch = fetch_values();
                if (rc_fetch) return rc_fetch;
                have_seed = info == 0;
                decided = info == 0 && loose && gram_values_decide(sv, max_bond_dim, abs_err, rel_err);
            }
            if (!decided) QSV_HIP(hipMemcpyAsync(theta, backup, sizeof(amp_t) * rows * cols, hipMemcpyDeviceToDevice, stream));
        }
    }
    if (!decided && jacobi_fits) {      // theta is intact here (zgesdd worked on it, but it was restored)
        const int own = jacobi_full_split(a, h, stream, theta, rows, cols, max_bond_dim, abs_err, rel_err, m1, m2, capacity,
                                          rank_out, s_host, buf, have_seed ? dU : nullptr, have_seed ? dV : nullptr);
        if (own != QSV_UNDECIDED) return own;
    }
    if (!decided) {
        const rocblas_status s = a.zgesvd(h, rocblas_svect_singular, rocblas_svect_singular, ci, ri, Z(theta), ci, dS, Z(dU),
                                          ci, Z(dV), ki, dE, rocblas_outofplace, dinfo);
        if (s != rocblas_status_success) return qsv_fail(QSV_EHIP, "rocsolver_zgesvd failed");
        const int rc_fetch = fetch_values();
        if (rc_fetch) return rc_fetch;
        if (info != 0) return qsv_fail(QSV_EHIP, "rocsolver_zgesvd did not converge");
    }
    const uint64_t r = kept_rank(sv, max_bond_dim, abs_err, rel_err);
    if (r > capacity) return qsv_fail(QSV_EINVAL, "output buffers are smaller than the kept bond dimension");
    if (r > 0) {
        hipLaunchKernelGGL(k_scale_columns, dim3(blocks_for(rows * r)), dim3(QSV_BLOCK), 0, stream, dV, m1, rows, k, r,
                           dS);
        hipLaunchKernelGGL(k_scale_rows, dim3(blocks_for(r * cols)), dim3(QSV_BLOCK), 0, stream, dU, m2, cols, r, dS);
        QSV_HIP(hipGetLastError());
        QSV_HIP(hipStreamSynchronize(stream));   // the factors are freed on return
    }
    if (s_host)
        for (uint64_t i = 0; i < k; ++i) s_host[i] = sv[i];
    *rank_out = r;
    return QSV_OK;
}

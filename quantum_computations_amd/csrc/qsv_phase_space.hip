// Phase-space read-out of CV registers: Wigner functions of sampled density matrices (utils.wigner) and the reduced
// density matrix of an MPS site on the device (SiteRegister.reduced_density_device).
//
// With hbar = 1 and rho sampled on x_k = x0 + k dx (k < d), the grid quadrature of
//     W(q, p) = (1/pi) int rho(q - y, q + y) e^{2ipy} dy
// substituting x = q - y is  W(q, p) = (dx/pi) Re sum_k rho(x_k, 2q - x_k) e^{2ip(q - x_k)},  where rho(x_k, .) is the
// Whittaker-Shannon interpolant of row k.  With s_q = 2(q - x0)/dx that is two products and an epilogue:
//     A[q, k] = sum_n G[q, n] R[n, k]      G[q, n] = sinc(s_q - n) (real, nq x (2d-1)), R[n, k] = rho[k, n-k] (0 <= n-k < d)
//     B[q, p] = sum_k A[q, k] E[k, p]      E[k, p] = e^{-2ip x_k}
//     W[p, q] = (dx/pi) Re(e^{2ipq} B[q, p])
// Both products run on one f64 MFMA kernel (v_mfma_f64_16x16x4f64) over real views:
//   * first product: G times [R_1 ... R_B] read as a (2d-1) x 2dB real matrix; R is never stored -- the B-operand tiles
//     are gathered from rho by address arithmetic, and a 32-column block of R is non-zero only for d + 31 of its
//     2d - 1 rows, which is all the K loop visits.  The output A (nq x 2dB) read as (nq B) x d complex rows is
//   * the second product's A operand: a complex product over k is a real one over 2k + c against the (2d x 2np) table
//     E2[2k + c, 2p + c'] = [[Re E, Im E], [-Im E, Re E]], so the real result IS the complex (nq B) x np matrix B.
// Every output element's K order depends only on its own column block, so a batch of B density matrices gives the
// bits of B separate calls.  When every s_q is an integer (q on the half-grid, e.g. q = the grid itself), G is a delta
// and A is gathered straight from rho (k_wigner_halfgrid) -- no first product.
//
// Workspace comes from the grow-only per-device pool of qsv_linalg.h; the call holds the library lock and ends with a
// stream synchronisation, as the pool's contract requires.
#include <cmath>
#include <cstring>
#include <mutex>

#include "qsv_linalg.h"

using namespace qsvl;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TM = 64;       // rows per workgroup tile
constexpr int TN = 64;       // real columns per workgroup tile
constexpr int TK = 16;       // inner-dimension step held in LDS
constexpr int PAD = 1;       // LDS row padding (doubles)

// C (M x N per batch, real, row-major, ldc) = A (M x K, lda) . B (K x N), on a 256-thread workgroup: four waves, each
// a 32 x 32 quarter of the 64 x 64 tile as 2 x 2 MFMA blocks.
//   GATHER = false: B is a plain row-major matrix (ldb), one batch.
//   GATHER = true:  B is [R_1 ... R_B] gathered from rho (batch x d x d complex); blockIdx.x = batch * tiles_per + tile,
//                   and the K loop covers only the band rows of the tile's 32 complex columns.
template <bool GATHER>
__global__ __launch_bounds__(256) void k_real_gemm(const double *__restrict__ A, uint64_t lda, const double *__restrict__ Bm,
                                                   uint64_t ldb, const amp_t *__restrict__ rho, uint64_t d,
                                                   double *__restrict__ C, uint64_t ldc, uint64_t M, uint64_t N, uint64_t K,
                                                   unsigned tiles_per_batch) {
    __shared__ double As[TK][TM + PAD];
    __shared__ double Bs[TK][TN + PAD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t row0 = static_cast<uint64_t>(blockIdx.y) * TM;
    const unsigned batch = GATHER ? blockIdx.x / tiles_per_batch : 0;
    const uint64_t col0 = static_cast<uint64_t>(GATHER ? blockIdx.x % tiles_per_batch : blockIdx.x) * TN;
    uint64_t k_begin = 0, k_end = K;
    const amp_t *rho_b = nullptr;
    if (GATHER) {
        // complex columns j0 .. j1-1 of R are non-zero in rows n = j .. j + d - 1
        const uint64_t j0 = col0 / 2, j1 = j0 + TN / 2 < d ? j0 + TN / 2 : d;
        k_begin = j0;
        k_end = j1 + d - 1 < K ? j1 + d - 1 : K;
        rho_b = rho + static_cast<uint64_t>(batch) * d * d;
    }
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (uint64_t k0 = k_begin; k0 < k_end; k0 += TK) {
        // A tile: lanes run along k (coalesced rows of A), stored k-major for the MFMA operand reads
#pragma unroll
        for (int i = 0; i < TM * TK / 256; ++i) {
            const int kk = t & (TK - 1), m = (t >> 4) + 16 * i;
            const uint64_t gr = row0 + m, gk = k0 + kk;
            As[kk][m] = (gr < M && gk < k_end) ? A[gr * lda + gk] : 0.0;
        }
        if (GATHER) {
            // R[n, j] = rho[j, n - j]: lanes run along n, i.e. along a row of rho
#pragma unroll
            for (int i = 0; i < TN / 2 * TK / 256; ++i) {
                const int kk = t & (TK - 1), jl = (t >> 4) + 16 * i;
                const uint64_t n = k0 + kk, j = col0 / 2 + jl;
                amp_t v = amp_t{0.0, 0.0};
                if (n < k_end && j < d && n >= j && n - j < d) v = rho_b[j * d + (n - j)];
                Bs[kk][2 * jl] = v.x;
                Bs[kk][2 * jl + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < TN * TK / 256; ++i) {
                const int c = t & (TN - 1), kk = (t >> 6) + 4 * i;
                const uint64_t gc = col0 + c, gk = k0 + kk;
                Bs[kk][c] = (gc < N && gk < k_end) ? Bm[gk * ldb + gc] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TK / 4; ++s) {
            const int kk = 4 * s + (lane >> 4);
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[kk][wm + 16 * i + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[kk][wn + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the f64 form: column lane & 15, row (lane >> 4) + 4 r
    const uint64_t out_col0 = GATHER ? static_cast<uint64_t>(batch) * N + col0 : col0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t gr = row0 + wm + 16 * i + (lane >> 4) + 4 * r;
                const uint64_t gc = col0 + wn + 16 * j + (lane & 15);
                if (gr < M && gc < N) C[gr * ldc + out_col0 + (gc - col0)] = acc[i][j][r];
            }
}

// G[q, n] = sinc(s_q - n) on n < 2d - 1, with sin(pi (s - n)) = (-1)^(i - n) sinpi(f) for s = i + f, i = rint(s):
// sin(M_PI * s) itself would lose digits at s ~ 2d.
__global__ __launch_bounds__(256) void k_sinc_table(const double *__restrict__ qs, uint64_t nq, uint64_t width, double x0,
                                                    double dx, double *__restrict__ G) {
    const uint64_t total = nq * width;
    for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < total; e += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t q = e / width, n = e % width;
        const double s = 2.0 * (qs[q] - x0) / dx;
        const double i = rint(s), f = s - i;
        const double diff = (i - static_cast<double>(n)) + f;
        double g;
        if (f == 0.0) {
            g = diff == 0.0 ? 1.0 : 0.0;
        } else {
            const double sign = fmod(fabs(i - static_cast<double>(n)), 2.0) == 0.0 ? 1.0 : -1.0;
            g = sign * sinpi(f) / (M_PI * diff);
        }
        G[e] = g;
    }
}

// E2[2k + c, 2p + c'] for E[k, p] = e^{-2ip x_k}: [[Re E, Im E], [-Im E, Re E]] (row-major, 2np columns).
__global__ __launch_bounds__(256) void k_phase_table(const double *__restrict__ ps, uint64_t np_, uint64_t d, double x0,
                                                     double dx, double *__restrict__ E2) {
    const uint64_t total = d * np_;
    for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < total; e += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t k = e / np_, p = e % np_;
        double sn, cs;
        sincos(2.0 * ps[p] * (x0 + static_cast<double>(k) * dx), &sn, &cs);
        const double re = cs, im = -sn;
        double *top = E2 + (2 * k) * (2 * np_) + 2 * p, *bottom = top + 2 * np_;
        top[0] = re;
        top[1] = im;
        bottom[0] = -im;
        bottom[1] = re;
    }
}

// Half-grid q (every s_q an integer): A[q, b, k] = rho_b[k, s_q - k], zero outside the grid.
__global__ __launch_bounds__(256) void k_wigner_halfgrid(const amp_t *__restrict__ rho, const double *__restrict__ qs,
                                                         uint64_t nq, uint64_t batch, uint64_t d, double x0, double dx,
                                                         amp_t *__restrict__ A) {
    const uint64_t total = nq * batch * d;
    for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < total; e += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t k = e % d, qb = e / d, b = qb % batch, q = qb / batch;
        const double s = rint(2.0 * (qs[q] - x0) / dx);
        const double m = s - static_cast<double>(k);
        amp_t v = amp_t{0.0, 0.0};
        if (m >= 0.0 && m < static_cast<double>(d)) v = rho[(b * d + k) * d + static_cast<uint64_t>(m)];
        A[e] = v;
    }
}

// scale[b] = (dx / pi) / (normalised ? dx Tr rho_b : 1); one workgroup per matrix, fixed summation order.
__global__ __launch_bounds__(256) void k_wigner_scale(const amp_t *__restrict__ rho, uint64_t d, double dx, int normalised,
                                                      double *__restrict__ scale) {
    __shared__ double red[4];
    const amp_t *r = rho + static_cast<uint64_t>(blockIdx.x) * d * d;
    double acc = 0.0;
    for (uint64_t k = threadIdx.x; k < d; k += 256) acc += r[k * d + k].x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double trace = (red[0] + red[1]) + (red[2] + red[3]);
        scale[blockIdx.x] = normalised ? (dx / M_PI) / (dx * trace) : dx / M_PI;
    }
}

// W[b, p, q] = scale[b] Re(e^{2ipq} B[(q, b), p]).
__global__ __launch_bounds__(256) void k_wigner_epilogue(const amp_t *__restrict__ Bq, const double *__restrict__ qs,
                                                         const double *__restrict__ ps, const double *__restrict__ scale,
                                                         uint64_t nq, uint64_t np_, uint64_t batch, double *__restrict__ W) {
    const uint64_t total = batch * np_ * nq;
    for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < total; e += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t q = e % nq, bp = e / nq, p = bp % np_, b = bp / np_;
        const amp_t v = Bq[(q * batch + b) * np_ + p];
        double sn, cs;
        sincos(2.0 * ps[p] * qs[q], &sn, &cs);
        W[e] = scale[b] * (cs * v.x - sn * v.y);
    }
}

// out[j, l, r] = in[l, j, r] (conj when `conj`): an (L, d, R) site with the physical index moved to the front.
__global__ __launch_bounds__(256) void k_axis_first(const amp_t *__restrict__ in, amp_t *__restrict__ out, uint64_t L,
                                                    uint64_t d, uint64_t R, int conj) {
    const uint64_t total = L * d * R;
    for (uint64_t e = blockIdx.x * 256ull + threadIdx.x; e < total; e += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t r = e % R, jl = e / R, j = jl % d, l = jl / d;
        amp_t v = in[e];
        if (conj) v.y = -v.y;
        out[(j * L + l) * R + r] = v;
    }
}

unsigned grid_for(uint64_t total, unsigned cap = 1u << 16) {
    const uint64_t g = (total + 255) / 256;
    return static_cast<unsigned>(g < 1 ? 1 : g > cap ? cap : g);
}

int check_launch() {
    QSV_HIP(hipGetLastError());
    return QSV_OK;
}

template <bool GATHER>
int launch_real_gemm(hipStream_t stream, const double *A, uint64_t lda, const double *B, uint64_t ldb, const amp_t *rho,
                     uint64_t d, double *C, uint64_t ldc, uint64_t M, uint64_t N, uint64_t K, unsigned batch) {
    const unsigned tiles_n = static_cast<unsigned>((N + TN - 1) / TN);
    const uint64_t tiles_m = (M + TM - 1) / TM;
    if (tiles_m > 65535 || static_cast<uint64_t>(tiles_n) * batch > 0x7fffffffull)
        return qsv_fail(QSV_EINVAL, "Wigner window too large for one launch");
    hipLaunchKernelGGL(k_real_gemm<GATHER>, dim3(tiles_n * batch, static_cast<unsigned>(tiles_m)), dim3(256), 0, stream, A,
                       lda, B, ldb, rho, d, C, ldc, M, N, K, tiles_n);
    return check_launch();
}

bool all_finite(const double *v, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

int qsv_tensor_wigner(int device, void *hip_stream, const void *dev_rho, int batch, uint64_t d, double x0, double dx,
                      const double *q, uint64_t nq, const double *p, uint64_t np_, int normalised, void *dev_w) {
    // every check before the first HIP call
    if (!dev_rho || !dev_w || !q || !p) return qsv_fail(QSV_EINVAL, "null pointer");
    if (device < 0 || device >= 16) return qsv_fail(QSV_EINVAL, "device index out of range");
    if (d < 2) return qsv_fail(QSV_EINVAL, "a Wigner function needs a grid of at least two points");
    if (d > (1u << 20)) return qsv_fail(QSV_EINVAL, "grid too large");
    if (batch < 1) return qsv_fail(QSV_EINVAL, "batch must be at least 1");
    if (nq < 1 || np_ < 1) return qsv_fail(QSV_EINVAL, "empty q or p window");
    if (nq > (1u << 24) || np_ > (1u << 24)) return qsv_fail(QSV_EINVAL, "q or p window too large");
    if (!std::isfinite(x0)) return qsv_fail(QSV_EINVAL, "grid origin is not finite");
    if (!(dx > 0.0) || !std::isfinite(dx)) return qsv_fail(QSV_EINVAL, "grid spacing must be positive and finite");
    if (!all_finite(q, nq) || !all_finite(p, np_)) return qsv_fail(QSV_EINVAL, "q and p must be finite");
    const double p_max = M_PI / (2.0 * dx);
    for (uint64_t i = 0; i < np_; ++i)
        if (std::fabs(p[i]) > p_max)
            return qsv_fail(QSV_EINVAL, "|p| = " + std::to_string(std::fabs(p[i])) + " exceeds the grid's limit pi/(2 dx) = " +
                                            std::to_string(p_max) + ": the quadrature would alias");
    // half-grid window: every s_q = 2(q - x0)/dx an integer (up to the rounding of a linspace grid)
    bool half_grid = true;
    for (uint64_t i = 0; i < nq && half_grid; ++i) {
        const double s = 2.0 * (q[i] - x0) / dx;
        half_grid = std::fabs(s - std::rint(s)) <= 1e-11;
    }

    const uint64_t B = static_cast<uint64_t>(batch);
    const uint64_t width = 2 * d - 1;                         // columns of G
    const size_t bytes_q = nq * 8, bytes_p = np_ * 8, bytes_scale = B * 8;
    const size_t bytes_g = half_grid ? 0 : nq * width * 8;
    const size_t bytes_a = nq * B * d * 16;                    // A: nq x (B 2d) real = (nq B) x d complex
    const size_t bytes_e = 2 * d * 2 * np_ * 8;
    const size_t bytes_b = nq * B * np_ * 16;
    auto pad = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t total = pad(bytes_q) + pad(bytes_p) + pad(bytes_scale) + pad(bytes_g) + pad(bytes_a) + pad(bytes_e) +
                         pad(bytes_b);

    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;
    DeviceBuffers buf;
    buf.reserve(*ctx, total);
    double *dq, *dp, *dscale, *dg = nullptr, *da, *de, *db;
    if (!buf.alloc(&dq, bytes_q) || !buf.alloc(&dp, bytes_p) || !buf.alloc(&dscale, bytes_scale) ||
        (!half_grid && !buf.alloc(&dg, bytes_g)) || !buf.alloc(&da, bytes_a) || !buf.alloc(&de, bytes_e) ||
        !buf.alloc(&db, bytes_b))
        return qsv_fail(QSV_ENOMEM, "Wigner workspace allocation failed");
    QSV_HIP(hipMemcpyAsync(dq, q, bytes_q, hipMemcpyHostToDevice, stream));
    QSV_HIP(hipMemcpyAsync(dp, p, bytes_p, hipMemcpyHostToDevice, stream));

    const amp_t *rho = static_cast<const amp_t *>(dev_rho);
    hipLaunchKernelGGL(k_wigner_scale, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, rho, d, dx, normalised, dscale);
    if ((rc = check_launch()) != QSV_OK) return rc;
    hipLaunchKernelGGL(k_phase_table, dim3(grid_for(d * np_)), dim3(256), 0, stream, dp, np_, d, x0, dx, de);
    if ((rc = check_launch()) != QSV_OK) return rc;
    if (half_grid) {
        hipLaunchKernelGGL(k_wigner_halfgrid, dim3(grid_for(nq * B * d)), dim3(256), 0, stream, rho, dq, nq, B, d, x0, dx,
                           reinterpret_cast<amp_t *>(da));
        if ((rc = check_launch()) != QSV_OK) return rc;
    } else {
        hipLaunchKernelGGL(k_sinc_table, dim3(grid_for(nq * width)), dim3(256), 0, stream, dq, nq, width, x0, dx, dg);
        if ((rc = check_launch()) != QSV_OK) return rc;
        // A (nq x 2dB) = G (nq x (2d-1)) . [R_1 ... R_B]
        if ((rc = launch_real_gemm<true>(stream, dg, width, nullptr, 0, rho, d, da, 2 * d * B, nq, 2 * d, width,
                                         static_cast<unsigned>(B))) != QSV_OK)
            return rc;
    }
    // B ((nq B) x 2np real = (nq B) x np complex) = A ((nq B) x 2d) . E2 (2d x 2np)
    if ((rc = launch_real_gemm<false>(stream, da, 2 * d, de, 2 * np_, nullptr, d, db, 2 * np_, nq * B, 2 * np_, 2 * d, 1)) !=
        QSV_OK)
        return rc;
    hipLaunchKernelGGL(k_wigner_epilogue, dim3(grid_for(B * np_ * nq)), dim3(256), 0, stream,
                       reinterpret_cast<const amp_t *>(db), dq, dp, dscale, nq, np_, B, static_cast<double *>(dev_w));
    if ((rc = check_launch()) != QSV_OK) return rc;
    QSV_HIP(hipStreamSynchronize(stream));      // the pool is free again only when the kernels are done
    return QSV_OK;
}

int qsv_tensor_axis_density(int device, void *hip_stream, const void *dev_z, const void *dev_t, uint64_t L, uint64_t d,
                            uint64_t R, void *dev_out) {
    if (!dev_z || !dev_t || !dev_out) return qsv_fail(QSV_EINVAL, "null pointer");
    if (L == 0 || d == 0 || R == 0) return qsv_fail(QSV_EINVAL, "empty tensor");
    const uint64_t lim = 0x7fffffffull;
    if (d > lim || L * R > lim) return qsv_fail(QSV_EINVAL, "tensor too large");
    RocblasApi &a = api();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;
    rocblas_handle h = handle_of(*ctx, &rc);
    if (!h) return rc;
    const size_t bytes = L * d * R * 16;
    DeviceBuffers buf;
    buf.reserve(*ctx, 2 * ((bytes + 255) / 256 * 256));
    amp_t *zf, *tf;
    if (!buf.alloc(&zf, bytes) || !buf.alloc(&tf, bytes)) return qsv_fail(QSV_ENOMEM, "workspace allocation failed");
    const unsigned grid = grid_for(L * d * R);
    hipLaunchKernelGGL(k_axis_first, dim3(grid), dim3(256), 0, stream, static_cast<const amp_t *>(dev_z), zf, L, d, R, 0);
    if ((rc = check_launch()) != QSV_OK) return rc;
    hipLaunchKernelGGL(k_axis_first, dim3(grid), dim3(256), 0, stream, static_cast<const amp_t *>(dev_t), tf, L, d, R, 1);
    if ((rc = check_launch()) != QSV_OK) return rc;
    // out (d x d, row-major) = Z' (d x LR) . conj(T')^T; column-major: out^T = conj(T') Z'^T, i.e. the (LR x d) buffer of
    // conj(T') read column-major is its transpose -> op T, and Z' likewise
    const rocblas_double_complex one{1.0, 0.0}, zero{0.0, 0.0};
    const rocblas_int n = static_cast<rocblas_int>(d), k = static_cast<rocblas_int>(L * R);
    const rocblas_status s = a.zgemm(h, rocblas_operation_transpose, rocblas_operation_none, n, n, k, &one,
                                     reinterpret_cast<const rocblas_double_complex *>(tf), k, 0,
                                     reinterpret_cast<const rocblas_double_complex *>(zf), k, 0, &zero,
                                     static_cast<rocblas_double_complex *>(dev_out), n, 0, 1);
    if (s != rocblas_status_success) return qsv_fail(QSV_EHIP, "rocblas_zgemm failed");
    QSV_HIP(hipStreamSynchronize(stream));
    return QSV_OK;
}

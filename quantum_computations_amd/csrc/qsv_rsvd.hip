// The randomized split of a matrix-product-state update and the verified low-rank route of the exact one.
//
//   qsvg_rsvd_split        randomized branch of tensor_svd (mps.py:5-50): hand-written f64 MFMA tall-skinny products
//                          (qsv_skinny.hip), CholeskyQR3 panels and Jacobi factor SVDs (qsv_panel.hip); rocBLAS / rocSOLVER
//                          as the fallback
//   try_verified_low_rank  a 64..256-probe range finder of its own, accepted only when the truncation rule provably gives
//                          the same rank as on the full spectrum (for qsvg_svd_split and for wide randomized splits)
#include <cstdio>
#include <memory>
#include <mutex>
#include <vector>

#include "qsv_linalg.h"

using namespace qsvl;
using namespace qsv_split_rules;

namespace {

// out (column-major n x m, ld n) = in (row-major n x m): LDS-tiled transpose of the element order
__global__ __launch_bounds__(256) void k_to_column_major(const amp_t *__restrict__ in, amp_t *__restrict__ out,
                                                        uint64_t n, uint64_t m) {
    __shared__ amp_t tile[16][17];
    const uint64_t tiles_m = (m + 15) / 16, tiles = tiles_m * ((n + 15) / 16);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = (t / tiles_m) * 16, c0 = (t % tiles_m) * 16;
        __syncthreads();
        if (r0 + ty < n && c0 + tx < m) tile[ty][tx] = in[(r0 + ty) * m + c0 + tx];
        __syncthreads();
        if (c0 + ty < m && r0 + tx < n) out[(c0 + ty) * n + r0 + tx] = tile[tx][ty];
    }
}

// out[a, b] (row-major A x B) = sqrt(s[by_row ? a : b]) * in[a * sa + b * sb]
__global__ __launch_bounds__(QSV_BLOCK) void k_scale_strided(const amp_t *__restrict__ in, amp_t *__restrict__ out,
                                                            uint64_t A, uint64_t B, uint64_t sa, uint64_t sb,
                                                            const double *__restrict__ s, int by_row) {
    const uint64_t total = A * B;
    for (uint64_t o = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t a = o / B, b = o % B;
        const double w = sqrt(s[by_row ? a : b]);
        const amp_t v = in[a * sa + b * sb];
        out[o] = amp_t{w * v.x, w * v.y};
    }
}

// out[a, b] (row-major A x B) = sqrt(s[by_row ? a : b]) * (conj ? conj(in[...]) : in[a * sa + b * sb])
__global__ __launch_bounds__(QSV_BLOCK) void k_scale_strided_conj(const amp_t *__restrict__ in, amp_t *__restrict__ out,
                                                                 uint64_t A, uint64_t B, uint64_t sa, uint64_t sb,
                                                                 const double *__restrict__ s, int by_row,
                                                                 int conjugate) {
    const uint64_t total = A * B;
    for (uint64_t o = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t a = o / B, b = o % B;
        const double w = sqrt(s[by_row ? a : b]);
        const amp_t v = in[a * sa + b * sb];
        out[o] = amp_t{w * v.x, conjugate ? -w * v.y : w * v.y};
    }
}

// out (column-major l x l) = transpose of in (column-major l x l);  conjugate != 0: out = conj(in) elementwise instead
__global__ __launch_bounds__(256) void k_small_reorder(const amp_t *__restrict__ in, amp_t *__restrict__ out, int l,
                                                      int conjugate) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < l * l; e += gridDim.x * 256) {
        const int i = e % l, k = e / l;
        const amp_t v = conjugate ? in[e] : in[static_cast<size_t>(i) * l + k];
        out[e] = conjugate ? amp_t{v.x, -v.y} : v;
    }
}

// T (n x l, column-major) = Q (n x l, column-major) * R^H with R (l x l) row-major: the projection coefficients
// Q^H A = R^H Qb^H of the range finder, folded into the left panel.
__global__ __launch_bounds__(256) void k_panel_times_rh(const amp_t *__restrict__ Q, const amp_t *__restrict__ R,
                                                        amp_t *__restrict__ T, uint64_t n, int l) {
    const uint64_t total = n * static_cast<uint64_t>(l);
    for (uint64_t o = blockIdx.x * 256ull + threadIdx.x; o < total; o += gridDim.x * 256ull) {
        const uint64_t i = o % n;
        const int k = static_cast<int>(o / n);
        double re = 0.0, im = 0.0;
        for (int p = 0; p < l; ++p) {
            const amp_t q = Q[i + static_cast<uint64_t>(p) * n], r = R[static_cast<size_t>(k) * l + p];
            re += q.x * r.x + q.y * r.y;     // q * conj(r)
            im += q.y * r.x - q.x * r.y;
        }
        T[o] = amp_t{re, im};
    }
}

// partials[block] = sum over a 16 x 16 tile of |A(i, j) - sum_k T(i, k) conj(Qb(j, k))|^2: the squared Frobenius norm
// of what the projection misses, entry by entry -- no subtraction of two nearly equal norms, so the result is good
// down to rounding level (~1e-15 ||A||) instead of ~1e-8 ||A||.  A(i, j) = theta[i * si + j * sj].
__global__ __launch_bounds__(256) void k_residual_partials(const amp_t *__restrict__ theta, uint64_t si, uint64_t sj,
                                                           const amp_t *__restrict__ T, const amp_t *__restrict__ Qb,
                                                           uint64_t n, uint64_t m, int l, double *__restrict__ partials) {
    __shared__ amp_t ts[16][17], qs[16][17];
    __shared__ double red[4];
    const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
    const uint64_t tiles_i = (n + 15) / 16, tiles_j = (m + 15) / 16;
    double sum = 0.0;
    for (uint64_t tile = blockIdx.x; tile < tiles_i * tiles_j; tile += gridDim.x) {
        const uint64_t i0 = (tile % tiles_i) * 16, j0 = (tile / tiles_i) * 16;
        const uint64_t i = i0 + ti, j = j0 + tj;
        double re = 0.0, im = 0.0;
        for (int k0 = 0; k0 < l; k0 += 16) {
            __syncthreads();
            // thread (ti, tj) stages T(i0 + ti, k0 + tj) and Qb(j0 + ti, k0 + tj)
            const int kk = k0 + tj;
            ts[tj][ti] = (i0 + ti < n && kk < l) ? T[i0 + ti + static_cast<uint64_t>(kk) * n] : amp_t{0.0, 0.0};
            qs[tj][ti] = (j0 + ti < m && kk < l) ? Qb[j0 + ti + static_cast<uint64_t>(kk) * m] : amp_t{0.0, 0.0};
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const amp_t t = ts[k][ti], q = qs[k][tj];
                re += t.x * q.x + t.y * q.y;     // t * conj(q)
                im += t.y * q.x - t.x * q.y;
            }
        }
        if (i < n && j < m) {
            const amp_t a = theta[i * si + j * sj];
            const double dr = a.x - re, di = a.y - im;
            sum += dr * dr + di * di;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// The randomized split with the fused panel kernels: same algorithm and random stream as below, but every
// re-orthonormalisation is 9 launches and the l x m projection is decomposed through B^H = Qb Rb and a Jacobi SVD of Rb.
// `verify` != null switches to the *verified low-rank* mode used by the exact split (see qsvg_svd_split): all l computed
// values are examined, the Frobenius norm of what the l-dimensional projection misses is known exactly
// (||A||_F^2 - sum sigma~_i^2), and the split is accepted only if the truncation rule provably gives the same rank as it
// would on the full spectrum; the function returns QSV_UNDECIDED otherwise and theta is untouched.
struct LowRankCheck {
    double frobenius_squared;   // ||theta||_F^2
    int64_t max_bond_dim;       // the caller's cap (k_keep only bounds what the projection may return)
    uint64_t full_rank;         // min(rows, cols)
    std::vector<double> *values;   // out: the kept spectrum padded with zeros to full_rank
};

int rsvd_split_fused(RocblasApi &a, rocblas_handle h, StreamContext &ctx, const amp_t *theta, uint64_t rows, uint64_t cols,
                     int64_t k_keep, int l, int q, const amp_t *omega, double abs_err, double rel_err, amp_t *m1, amp_t *m2,
                     uint64_t capacity, uint64_t *rank_out, double *s_host, const LowRankCheck *verify = nullptr) {
    hipStream_t stream = ctx.stream;
    const bool trace = split_options().trace;
    const bool wide = rows < cols;
    const uint64_t n = wide ? cols : rows, m = wide ? rows : cols;
    const uint64_t L = static_cast<uint64_t>(l);
    DeviceBuffers buf;
    const uint64_t block = L < LMAX ? L : LMAX, scratch_amps = 2 * LMAX * LMAX;
    // the k-range shares of the skinny products: only matrices with few 64-row blocks use them (see skinny_gemm)
    const uint64_t share_amps = n < 256 * 64 ? SKINNY_MAX_SHARES * n * (L < 64 ? L : 64) : 0;
    buf.reserve(ctx, sizeof(amp_t) * ((n + m) * (L + static_cast<uint64_t>(k_keep)) + (verify ? n * L : 0) + share_amps +
                                         GRAM_BLOCKS * block * block + scratch_amps + 5 * L * L) + 32 * L + 16384 + 8 * 1024);
    amp_t *Qn = nullptr, *Qm = nullptr, *partials = nullptr, *small = nullptr, *UA = nullptr, *VA = nullptr, *shares = nullptr;
    double *dS = nullptr;
    // small: block scratch (2 x 64 x 64) | r_total | U_r | V_r | library scratch, each L x L
    if (!buf.alloc(&Qn, sizeof(amp_t) * n * L) || !buf.alloc(&Qm, sizeof(amp_t) * m * L) ||
        !buf.alloc(&partials, sizeof(amp_t) * GRAM_BLOCKS * block * block) ||
        !buf.alloc(&small, sizeof(amp_t) * (scratch_amps + 5 * L * L)) || !buf.alloc(&dS, sizeof(double) * (2 * L + 6)) ||
        (share_amps && !buf.alloc(&shares, sizeof(amp_t) * share_amps)))
        return qsv_fail(QSV_ENOMEM, "device allocation of the randomized-SVD workspace failed");
    amp_t *r_factor = small, *r_total = small + scratch_amps, *Ur = r_total + L * L, *Vr = Ur + L * L, *lib = Vr + L * L;
    int *flags = reinterpret_cast<int *>(dS + 2 * L + 2);     // round-skipping flags of the panel kernels (4 ints)
    // theta is row-major (rows x cols); read column-major it is M = theta^T (cols x rows, ld cols).  The reference works on
    // the tall orientation A: wide theta -> A = theta^T = M itself; tall theta -> A = theta = M^T, reached through the
    // transposed / conjugated forms of the panel kernels, so no re-ordered copy of theta is ever made.
    const amp_t *M = theta;
    const rocblas_int ni = static_cast<rocblas_int>(n), mi = static_cast<rocblas_int>(m), li = static_cast<rocblas_int>(L);
    auto gemm = [&](auto... args) { return zgemm(a, h, args...); };
    const rocblas_operation N = rocblas_operation_none, Cc = rocblas_operation_conjugate_transpose;
    // the passes over A: the MFMA panel kernels (l tiled by 16); rocBLAS if they decline the shape
    const rocblas_operation T_ = rocblas_operation_transpose;
    const rocblas_int ld = static_cast<rocblas_int>(cols);       // leading dimension of M
    auto times_a = [&](const amp_t *panel, amp_t *out) {          // out (n x l) = A panel (m x l)
        if (wide)   // A = M (n x m)
            return skinny_gemm(stream, false, false, M, panel, out, n, m, l, shares, share_amps) ||
                   gemm(N, N, ni, li, mi, M, ld, panel, mi, out, ni);
        // A = M^T with M (m x n)
        return skinny_gemm(stream, true, false, M, panel, out, m, n, l, shares, share_amps) || gemm(T_, N, ni, li, mi, M, ld, panel, mi, out, ni);
    };
    auto times_ah = [&](const amp_t *panel, amp_t *out) {         // out (m x l) = A^H panel (n x l)
        if (wide) return skinny_gemm(stream, true, true, M, panel, out, n, m, l, shares, share_amps) ||
                         gemm(Cc, N, mi, li, ni, M, ld, panel, ni, out, mi);
        // A^H = conj(M): no library form for a plain conjugate, the kernels take every l <= 64 this path is entered with
        return skinny_gemm(stream, false, true, M, panel, out, m, n, l, shares, share_amps);
    };
    const int between = split_options().panel_rounds;      // rounds of the panels in between (QSV_PANEL_ROUNDS=3: as the final ones)
    bool ok = times_a(omega, Qn);                                                                 // Y = A O
    int rc = ok ? wide_panel_orthonormalise(stream, Qn, n, l, partials, r_factor, nullptr, flags, q > 0 ? between : 3) : QSV_OK;
    for (int it = 0; ok && !rc && it < q; ++it) {
        ok = times_ah(Qn, Qm);                                                                    // Y = A^H Q
        if (ok) rc = wide_panel_orthonormalise(stream, Qm, m, l, partials, r_factor, nullptr, flags, between);
        ok = ok && !rc && times_a(Qm, Qn);                                                        // Y = A Q
        if (ok) rc = wide_panel_orthonormalise(stream, Qn, n, l, partials, r_factor, nullptr, flags, it + 1 < q ? between : 3);
    }
    // B^H = A^H Q = Qb Rb  (m x l);  Rb = Ur S Vr^H;  A ~ (Q Vr) S (Qb Ur)^H
    ok = ok && !rc && times_ah(Qn, Qm);
    if (ok) rc = wide_panel_orthonormalise(stream, Qm, m, l, partials, r_factor, r_total, flags);
    if (!ok) return qsv_fail(QSV_EHIP, "rocBLAS call failed in the randomized range finder");
    if (rc) return rc;
    const int rc_svd = factor_svd(stream, r_total, l, lib, Ur, dS, Vr, flags + 3);
    if (rc_svd) return rc_svd;
    const uint64_t k = verify ? L : static_cast<uint64_t>(k_keep);
    std::vector<double> sv(k);
    QSV_HIP(hipMemcpyAsync(sv.data(), dS, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipStreamSynchronize(stream));
    uint64_t r;
    if (verify) {
        // rho^2 = ||A||_F^2 - sum sigma~_i^2 is what the projection misses (low_rank_settled); the difference itself is
        // resolved down to ~1e-8 ||A||
        double captured = 0.0;
        for (double v : sv) captured += v * v;
        const double f2 = verify->frobenius_squared;
        double rho2 = f2 - captured;
        double resolution = 4e-16 * static_cast<double>(L) * f2;
        LowRankVerdict v{};
        // the acceptance test for a given bound on the missed mass: true = the rank is settled (v.r)
        auto settled_with = [&](double rho2_bound) {
            v = low_rank_settled(sv, rho2_bound, verify->full_rank, verify->max_bond_dim, k_keep, abs_err, rel_err);
            if (trace)
                fprintf(stderr, "[qsv split] %llu x %llu: probes %d, ||A||_F %.3e, rho %.3e, allowed %.3e, margin %.3e, s0 %.3e\n",
                        static_cast<unsigned long long>(rows), static_cast<unsigned long long>(cols), l, sqrt(f2), v.rho, v.allowed,
                        v.margin, sv[0]);
            if (trace && v.compared)
                fprintf(stderr, "[qsv split]   r in [%llu, %llu], s[r-1] %.3e\n", static_cast<unsigned long long>(v.r_lo),
                        static_cast<unsigned long long>(v.r_hi), v.r_lo > 0 ? sv[v.r_lo - 1] : 0.0);
            return v.settled;
        };
        bool settled = false;
        if (rho2 < 1e-6 * f2) {
            // The difference of the two norms is blind below ~1e-8 ||A||.  Under a loose tolerance that is still far more
            // than the test needs: try it with the blind spot itself as the bound -- a wider margin can only leave the
            // rank undecided, never change it (both thresholds move outwards) -- and only if that fails ...
            settled = settled_with(rho2 > resolution ? rho2 : resolution);
        }
        if (!settled && rho2 < 1e-6 * f2) {
            // ... (a tight tolerance: the reference's default rel_err = 1e-12) evaluate the residual itself:
            // (I - Q Q^H) A = A - (Q Rb^H) Qb^H entry by entry (A^H Q = Qb Rb was formed above), one l-term dot product
            // per entry, rounding level ~l eps ||A||.
            amp_t *Tp = nullptr;
            double *res_partials = nullptr;
            if (buf.alloc(&Tp, sizeof(amp_t) * n * L) && buf.alloc(&res_partials, sizeof(double) * 1024)) {
                hipLaunchKernelGGL(k_panel_times_rh, dim3(blocks_for(n * L)), dim3(256), 0, stream, Qn, r_total, Tp, n, l);
                // A(i, j): wide theta -> A = theta^T: theta[j * cols + i]; tall theta -> A = theta: theta[i * cols + j]
                hipLaunchKernelGGL(k_residual_partials, dim3(1024), dim3(256), 0, stream, theta, wide ? 1ull : cols,
                                   wide ? cols : 1ull, Tp, Qm, n, m, l, res_partials);
                QSV_HIP(hipGetLastError());
                std::vector<double> parts(1024);
                QSV_HIP(hipMemcpyAsync(parts.data(), res_partials, sizeof(double) * 1024, hipMemcpyDeviceToHost, stream));
                QSV_HIP(hipStreamSynchronize(stream));
                double explicit_rho2 = 0.0;
                for (double v : parts) explicit_rho2 += v;
                rho2 = explicit_rho2;
                // rounding floor of the entry-wise evaluation: each entry carries ~sqrt(l) eps |A_ij| (random signs)
                resolution = 1e-30 * static_cast<double>(L) * f2;
            }
        }
        if (!settled) settled = settled_with(rho2 > resolution ? rho2 : resolution);
        if (!settled) return QSV_UNDECIDED;
        r = v.r;
        if (verify->values) {
            verify->values->assign(verify->full_rank, 0.0);
            for (uint64_t i = 0; i < L && i < verify->full_rank; ++i) (*verify->values)[i] = sv[i];
        }
    } else {
        r = kept_rank(sv, k_keep, abs_err, rel_err);
    }
    if (r > capacity) return qsv_fail(QSV_EINVAL, "output buffers are smaller than the kept bond dimension");
    if (r > 0) {
        const rocblas_int ri = static_cast<rocblas_int>(r);
        if (!buf.alloc(&UA, sizeof(amp_t) * n * r) || !buf.alloc(&VA, sizeof(amp_t) * m * r))
            return qsv_fail(QSV_ENOMEM, "device allocation of the randomized-SVD workspace failed");
        if (!gemm(N, N, ni, ri, li, Qn, ni, Vr, li, UA, ni) || !gemm(N, N, mi, ri, li, Qm, mi, Ur, li, VA, mi))
            return qsv_fail(QSV_EHIP, "rocblas_zgemm failed");
        // A = UA S VA^H.  Tall theta = A:  m1 = UA sqrt(S),  m2 = sqrt(S) VA^H.
        // Wide theta = A^T = conj(VA) S UA^T:  m1 = conj(VA) sqrt(S),  m2 = sqrt(S) UA^T.
        const amp_t *u_src = wide ? VA : UA, *v_src = wide ? UA : VA;
        const uint64_t u_ld = wide ? m : n, v_ld = wide ? n : m;
        hipLaunchKernelGGL(k_scale_strided_conj, dim3(blocks_for(rows * r)), dim3(QSV_BLOCK), 0, stream, u_src, m1, rows,
                           r, static_cast<uint64_t>(1), u_ld, dS, 0, wide ? 1 : 0);
        hipLaunchKernelGGL(k_scale_strided_conj, dim3(blocks_for(r * cols)), dim3(QSV_BLOCK), 0, stream, v_src, m2, r,
                           cols, v_ld, static_cast<uint64_t>(1), dS, 1, wide ? 0 : 1);
        QSV_HIP(hipGetLastError());
    }
    QSV_HIP(hipStreamSynchronize(stream));   // the workspace is freed on return
    if (s_host && !verify)
        for (uint64_t i = 0; i < k; ++i) s_host[i] = sv[i];
    *rank_out = r;
    return QSV_OK;
}

// sum of |x|^2 over `count` amplitudes into per-block partials
__global__ __launch_bounds__(256) void k_sum_squares(const amp_t *__restrict__ x, uint64_t count, double *__restrict__ partials) {
    __shared__ double red[4];
    double s = 0.0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < count; i += gridDim.x * 256ull) s += x[i].x * x[i].x + x[i].y * x[i].y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// The probe matrices of the verified low-rank route, per device, width and matrix size: they depend only on those (a
// fixed random stream), so every stream shares them.  (Several sizes per width: the thetas of one MPS alternate between a
// few shapes -- 1000, 2000, 4000 on the short side in the GKP runs -- and with ONE entry per width every change of shape
// cost a Box-Muller pass over 10^5 deviates on the host, an allocation and an upload.)  Entries are handed out
// reference-counted, and an evicted entry is kept in `retired` until qsv_tensor_release_workspace: a split on another
// stream may still read it, and hipFree would wait for the whole device.
struct ProbeMatrix {
    amp_t *omega = nullptr;
    uint64_t count = 0;
    ~ProbeMatrix() {
        if (omega) (void)hipFree(omega);
    }
};

struct ProbeCache {
    static constexpr int SIZES = 8;
    struct Slot {
        std::shared_ptr<ProbeMatrix> probes;
        uint64_t last_use = 0;
    };
    std::mutex lock;          // held for lookup and insertion only
    Slot slots[16][3][SIZES];
    std::vector<std::shared_ptr<ProbeMatrix>> retired[16];
    uint64_t use_clock = 0;
};

ProbeCache &probe_cache() {
    static ProbeCache *c = new ProbeCache;     // never destroyed: no hipFree after the runtime has gone at exit
    return *c;
}

// The (full x l) probe matrix of width index `w` on the context's device, generated and uploaded on the context's stream
// when no stream has it yet; null when the device memory is not there.
std::shared_ptr<ProbeMatrix> probes_for(StreamContext &ctx, int w, uint64_t full, int l) {
    ProbeCache &cache = probe_cache();
    ProbeCache::Slot *row = cache.slots[ctx.device][w];
    const uint64_t count = full * static_cast<uint64_t>(l);
    {
        std::lock_guard<std::mutex> guard(cache.lock);
        for (int i = 0; i < ProbeCache::SIZES; ++i)
            if (row[i].probes && row[i].probes->count == count) {
                row[i].last_use = ++cache.use_clock;
                return row[i].probes;
            }
    }
    auto fresh = std::make_shared<ProbeMatrix>();
    if (hipMalloc(reinterpret_cast<void **>(&fresh->omega), sizeof(amp_t) * count) != hipSuccess) {
        fresh->omega = nullptr;
        (void)hipGetLastError();
        return nullptr;
    }
    std::vector<double> host(2 * count, 0.0);
    uint64_t state = 0x9e3779b97f4a7c15ull + static_cast<uint64_t>(w);   // splitmix64 + Box-Muller: fixed probe matrices
    auto next = [&]() {
        state += 0x9e3779b97f4a7c15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return ((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
    };
    for (uint64_t i = 0; i < count; ++i) {
        const double u1 = next() + 1e-300, u2 = next();
        host[2 * i] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    }
    // complete before it is published (a synchronous copy): other streams may use the entry as soon as it is in the cache
    if (hipMemcpy(fresh->omega, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    fresh->count = count;
    std::lock_guard<std::mutex> guard(cache.lock);
    ProbeCache::Slot *slot = nullptr;
    for (int i = 0; i < ProbeCache::SIZES; ++i)
        if (row[i].probes && row[i].probes->count == count) slot = &row[i];      // another stream was quicker: use its copy
    if (slot) {
        slot->last_use = ++cache.use_clock;
        cache.retired[ctx.device].push_back(std::move(fresh));    // never published; freed with the other retired ones
        return slot->probes;
    }
    slot = &row[0];                          // a free entry, or the one that was used longest ago
    for (int i = 0; i < ProbeCache::SIZES; ++i)
        if (!row[i].probes) {
            slot = &row[i];
            break;
        } else if (row[i].last_use < slot->last_use) {
            slot = &row[i];
        }
    if (slot->probes) cache.retired[ctx.device].push_back(std::move(slot->probes));
    slot->probes = fresh;
    slot->last_use = ++cache.use_clock;
    return fresh;
}

}  // namespace

// Free the probe matrices evicted on `device` (qsv_tensor_release_workspace, after it has waited for the device).
int release_retired_probes(int device) {
    std::vector<std::shared_ptr<ProbeMatrix>> gone;
    {
        ProbeCache &cache = probe_cache();
        std::lock_guard<std::mutex> guard(cache.lock);
        gone.swap(cache.retired[device]);
    }
    gone.clear();
    return QSV_OK;
}

// The exact split's shortcut for numerically low-rank theta under a loose tolerance (the regime of the reference's own
// GKP runs: rel_err = 1e-2, bonds of 1-2 on d = 1000 grids, where LAPACK-style SVDs of 1000..2000-sized matrices are all
// the time there is): a 64-probe range finder with its own fixed random stream -- the reference's exact branch draws no
// random numbers, so the caller's generator must not be touched -- verified a posteriori by LowRankCheck.
int qsvl::try_verified_low_rank(RocblasApi &a, rocblas_handle h, StreamContext &ctx, const amp_t *theta, uint64_t rows,
                                uint64_t cols, int64_t max_bond_dim, double abs_err, double rel_err, amp_t *m1, amp_t *m2,
                                uint64_t capacity, uint64_t *rank_out, double *s_host, uint64_t s_count,
                                double *frobenius_squared_out) {
    const uint64_t full = rows < cols ? rows : cols;
    if (full < 4 * static_cast<uint64_t>(LMAX)) return QSV_UNDECIDED;    // small matrices: the library SVD is cheap
    // the norm partials live outside the pool (which rsvd_split_fused carves for itself), in the stream's context; the
    // probe matrices in the cache shared by every stream of the device (probes_for)
    hipStream_t stream = ctx.stream;
    if (!ctx.norm_partials &&
        hipMalloc(reinterpret_cast<void **>(&ctx.norm_partials), sizeof(double) * 256) != hipSuccess) {
        ctx.norm_partials = nullptr;
        (void)hipGetLastError();
        return QSV_UNDECIDED;
    }
    double *partials = ctx.norm_partials;
    hipLaunchKernelGGL(k_sum_squares, dim3(256), dim3(256), 0, stream, theta, rows * cols, partials);
    QSV_HIP(hipGetLastError());
    double sums[256];
    QSV_HIP(hipMemcpyAsync(sums, partials, sizeof(sums), hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipStreamSynchronize(stream));
    std::vector<double> spectrum;       // the computed values of the attempt that decided (padded with zeros to `full`)
    LowRankCheck check{0.0, max_bond_dim, full, &spectrum};
    for (double v : sums) check.frobenius_squared += v;
    if (frobenius_squared_out) *frobenius_squared_out = check.frobenius_squared;
    if (!(check.frobenius_squared > 0.0)) return QSV_UNDECIDED;
    // One 64-column block of probes keeps everything in the fused kernels; when the numerical rank does not fit (the kept
    // triplets must leave ten probes of oversampling and stand well above what was missed) the panel is widened to 128 and
    // 256 probes (64-column blocks, Jacobi sweeps in global memory) before the library SVD gets the matrix: even the
    // widest attempt costs tens of milliseconds where zgesvd takes seconds on these graded spectra.
    // (Starting at the width that decided the last split of the same shape was measured on the 15 dB GKP Grover run: 3.5 s
    // against 3.3 -- a 128-probe attempt costs three to four 64-probe ones, and most splits still pass at 64.)
    const int widths[3] = {LMAX, 2 * LMAX, WIDE_MAX};
    for (int w = 0; w < 3; ++w) {
        const int l = widths[w], keep = l - 10;
        if (full < 4 * static_cast<uint64_t>(l)) break;
        const std::shared_ptr<ProbeMatrix> probes = probes_for(ctx, w, full, l);
        if (!probes) return QSV_UNDECIDED;
        // two power iterations: the route is accepted only when the kept values stand 10^2 rho above everything that was
        // missed, and the error of their subspace after q iterations is of order (missed / kept)^(2q+1)
        const int rc = rsvd_split_fused(a, h, ctx, theta, rows, cols, keep, l, 2, probes->omega, abs_err, rel_err, m1, m2,
                                        capacity, rank_out, nullptr, &check);
        if (rc == QSV_OK && s_host)
            for (uint64_t i = 0; i < s_count; ++i) s_host[i] = spectrum[i];
        if (rc != QSV_UNDECIDED) return rc;
    }
    return QSV_UNDECIDED;
}

// tensor_svd on its randomized branch (mps.py:5-50,78-79; Halko, Martinsson & Tropp 2010): range finder with
// l = k + 10 Gaussian probes (drawn by the caller so that the reference's random stream is reproduced) and q power
// iterations re-orthonormalised by Householder QR, SVD of the small l x m' projection, first k triplets kept, then the
// same truncation rule.  Everything is column-major here; A is the tall orientation of theta (the reference
// transposes a wide matrix first) and `omega` is (m' x l) column-major, m' = min(rows, cols).
int qsvg_rsvd_split(int device, hipStream_t stream, const amp_t *theta, uint64_t rows, uint64_t cols, int64_t k_keep,
                    int l, int q, const amp_t *omega, double abs_err, double rel_err, amp_t *m1, amp_t *m2,
                    uint64_t capacity, uint64_t *rank_out, double *s_host) {
    const uint64_t lim = 0x7fffffffull;
    if (rows > lim || cols > lim) return qsv_fail(QSV_EINVAL, "matrix dimension exceeds 2^31 - 1");
    RocblasApi &a = api();
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;
    rocblas_handle h = handle_of(*ctx, &rc);
    if (!h) return rc;
    if (!a.zgesvd || !a.zgeqrf || !a.zungqr)
        return qsv_fail(QSV_EHIP, "rocSOLVER could not be loaded (librocsolver.so.0): no SVD available");
    const bool wide = rows < cols;                      // the reference works on theta^T then
    const uint64_t n = wide ? cols : rows, m = wide ? rows : cols;   // A is n x m, n >= m
    const uint64_t L = static_cast<uint64_t>(l), kk = L < m ? L : m;
    if (k_keep < 1 || L < static_cast<uint64_t>(k_keep) || L > m)
        return qsv_fail(QSV_EINVAL, "need 1 <= k <= l <= min(rows, cols)");
    const SplitOptions &opt = split_options();
    if (omega && L <= LMAX && opt.fused_panels)
        return rsvd_split_fused(a, h, *ctx, theta, rows, cols, k_keep, l, q, omega, abs_err, rel_err, m1, m2, capacity,
                                rank_out, s_host);
    // More probes than the fused kernels take (max_bond_dim > 54, e.g. the 100 of the reference's GKP runs).  Under a
    // loose tolerance the kept rank is far below that anyway: the verified low-rank route decides it with 64 probes of
    // its own; the caller has already drawn -- and thereby consumed from its generator -- the test matrix the reference
    // would use, so the random stream of a seeded simulation is unaffected.
    // A caller that came without its test matrix, was asked for it and is back with it (same theta, untouched in between)
    // has had its verified attempts already: do not repeat them.  (The memo is the stream's: the second call comes on
    // the stream of the first.)
    const bool back_with_omega = omega && ctx->asked_theta == theta && ctx->asked_rows == rows && ctx->asked_cols == cols;
    ctx->asked_theta = nullptr;
    if (!back_with_omega && L > LMAX && opt.shortcuts && opt.fused_panels && (rel_err >= 1e-4 || abs_err > 0.0)) {
        const int fast = try_verified_low_rank(a, h, *ctx, theta, rows, cols, k_keep, abs_err, rel_err, m1, m2, capacity,
                                               rank_out, s_host, static_cast<uint64_t>(k_keep));
        if (fast != QSV_UNDECIDED) return fast;
    }
    if (!omega) {      // the caller has not drawn the test matrix yet (it costs more than the route above): ask for it
        ctx->asked_theta = theta;
        ctx->asked_rows = rows;
        ctx->asked_cols = cols;
        *rank_out = QSV_RANK_NEEDS_OMEGA;
        return QSV_OK;
    }
    if (L <= WIDE_MAX && opt.fused_panels)      // 64-column blocks of probes, library SVD of the projected factor
        return rsvd_split_fused(a, h, *ctx, theta, rows, cols, k_keep, l, q, omega, abs_err, rel_err, m1, m2, capacity,
                                rank_out, s_host);
    DeviceBuffers buf;
    buf.reserve(*ctx, sizeof(amp_t) * ((n + m) * L + L + L * m + L * kk + kk * m + n * static_cast<uint64_t>(k_keep) +
                                         (wide ? 0 : n * m)) + 16 * kk + 8192);
    amp_t *A = nullptr, *Qn = nullptr, *Qm = nullptr, *tau = nullptr, *B = nullptr, *UB = nullptr, *VB = nullptr;
    double *dS = nullptr, *dE = nullptr;
    rocblas_int *dinfo = nullptr;
    if (!buf.alloc(&Qn, sizeof(amp_t) * n * L) || !buf.alloc(&Qm, sizeof(amp_t) * m * L) ||
        !buf.alloc(&tau, sizeof(amp_t) * L) || !buf.alloc(&B, sizeof(amp_t) * L * m) ||
        !buf.alloc(&UB, sizeof(amp_t) * L * kk) || !buf.alloc(&VB, sizeof(amp_t) * kk * m) ||
        !buf.alloc(&dS, sizeof(double) * (2 * kk + 2)))
        return qsv_fail(QSV_ENOMEM, "device allocation of the randomized-SVD workspace failed");
    dE = dS + kk;
    dinfo = reinterpret_cast<rocblas_int *>(dS + 2 * kk);
    if (wide) {
        // theta row-major (rows x cols) read column-major is theta^T (cols x rows) = A already
        A = const_cast<amp_t *>(theta);
    } else {
        if (!buf.alloc(&A, sizeof(amp_t) * n * m))
            return qsv_fail(QSV_ENOMEM, "device allocation of the randomized-SVD workspace failed");
        const uint64_t tiles = ((n + 15) / 16) * ((m + 15) / 16);
        hipLaunchKernelGGL(k_to_column_major, dim3(static_cast<unsigned>(tiles < 65536 ? tiles : 65536)), dim3(256), 0,
                           stream, theta, A, n, m);
        QSV_HIP(hipGetLastError());
    }
    const rocblas_int ni = static_cast<rocblas_int>(n), mi = static_cast<rocblas_int>(m), li = static_cast<rocblas_int>(L);
    auto gemm = [&](auto... args) { return zgemm(a, h, args...); };
    auto orthonormalise = [&](amp_t *Y, rocblas_int rows_) {      // Y <- Q of its reduced QR
        return a.zgeqrf(h, rows_, li, Z(Y), rows_, Z(tau)) == rocblas_status_success &&
               a.zungqr(h, rows_, li, li, Z(Y), rows_, Z(tau)) == rocblas_status_success;
    };
    const rocblas_operation N = rocblas_operation_none, Cc = rocblas_operation_conjugate_transpose;
    bool ok = gemm(N, N, ni, li, mi, A, ni, omega, mi, Qn, ni) && orthonormalise(Qn, ni);       // Y = A O
    for (int it = 0; ok && it < q; ++it) {
        ok = gemm(Cc, N, mi, li, ni, A, ni, Qn, ni, Qm, mi) && orthonormalise(Qm, mi) &&         // Y = A^H Q
             gemm(N, N, ni, li, mi, A, ni, Qm, mi, Qn, ni) && orthonormalise(Qn, ni);            // Y = A Q
    }
    ok = ok && gemm(Cc, N, li, mi, ni, Qn, ni, A, ni, B, li);                                    // B = Q^H A  (l x m)
    if (!ok) return qsv_fail(QSV_EHIP, "rocBLAS / rocSOLVER call failed in the randomized range finder");
    if (a.zgesvd(h, rocblas_svect_singular, rocblas_svect_singular, li, mi, Z(B), li, dS, Z(UB), li, Z(VB),
                 static_cast<rocblas_int>(kk), dE, rocblas_outofplace, dinfo) != rocblas_status_success)
        return qsv_fail(QSV_EHIP, "rocsolver_zgesvd failed");
    const uint64_t k = static_cast<uint64_t>(k_keep);
    std::vector<double> sv(k);
    rocblas_int info = 0;
    QSV_HIP(hipMemcpyAsync(sv.data(), dS, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipMemcpyAsync(&info, dinfo, sizeof(info), hipMemcpyDeviceToHost, stream));
    QSV_HIP(hipStreamSynchronize(stream));
    if (info != 0) return qsv_fail(QSV_EHIP, "rocsolver_zgesvd did not converge");
    const uint64_t r = kept_rank(sv, k_keep, abs_err, rel_err);
    if (r > capacity) return qsv_fail(QSV_EINVAL, "output buffers are smaller than the kept bond dimension");
    if (r > 0) {
        // U_A = Q U_B[:, :r]  (n x r, column-major)
        amp_t *UA = nullptr;
        if (!buf.alloc(&UA, sizeof(amp_t) * n * r))
            return qsv_fail(QSV_ENOMEM, "device allocation of the randomized-SVD workspace failed");
        if (!gemm(N, N, ni, static_cast<rocblas_int>(r), li, Qn, ni, UB, li, UA, ni))
            return qsv_fail(QSV_EHIP, "rocblas_zgemm failed");
        // A = U_A S Vh_B.  Tall theta: theta = A; wide theta: theta = A^T = Vh_B^T S U_A^T.
        const amp_t *u_src = wide ? VB : UA, *v_src = wide ? UA : VB;
        // m1[row, i] = sqrt(s_i) u[row, i];  m2[i, c] = sqrt(s_i) vh[i, c]
        const uint64_t u_sa = wide ? kk : 1, u_sb = wide ? 1 : n;          // wide: u[row, i] = VB[i + row * kk]
        const uint64_t v_sa = wide ? n : 1, v_sb = wide ? 1 : kk;          // wide: vh[i, c] = UA[c + i * n]
        hipLaunchKernelGGL(k_scale_strided, dim3(blocks_for(rows * r)), dim3(QSV_BLOCK), 0, stream, u_src, m1, rows, r,
                           u_sa, u_sb, dS, 0);
        hipLaunchKernelGGL(k_scale_strided, dim3(blocks_for(r * cols)), dim3(QSV_BLOCK), 0, stream, v_src, m2, r, cols,
                           v_sa, v_sb, dS, 1);
        QSV_HIP(hipGetLastError());
    }
    QSV_HIP(hipStreamSynchronize(stream));   // the workspace is freed on return
    if (s_host)
        for (uint64_t i = 0; i < k; ++i) s_host[i] = sv[i];
    *rank_out = r;
    return QSV_OK;
}

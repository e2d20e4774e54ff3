// Multi-register BLAS-1 passes of the qubit register (gfx950, wave64) and their C entry points: qsv_lincomb
// (dst = beta dst + sum_k c_k src_k, optionally with ||dst||^2 of what it stores) and qsv_inner_many (<x_k|y> for many
// x_k in shared passes over y).  The pieces Krylov methods on a Pauli sum need next to qsv_apply_pauli_sum (DESIGN.md
// section 19).  Pure streaming kernels: one 16-byte load per operand and amplitude, no LDS except in the reductions.
// Passes, grids and the slices of the scratch buffer come from qsv_krylov_layout.h.

#include "qsv_device.h"
#include "qsv_krylov_layout.h"

#include <cstring>
#include <vector>

using namespace qsv_krylov_layout;

static_assert(KRYLOV_BLOCK == QSV_BLOCK && KRYLOV_REDUCE_BLOCKS == QSV_REDUCE_BLOCKS, "qsv_krylov_layout.h mirrors qsv_internal.h");

namespace {

// dst[i] = beta dst[i] + sum_{k < K} c_k src_k[i].  Exactly K source streams: slot k >= K of the arguments is never
// touched.  BETA: the pass's beta is not exactly 0 and the old dst is loaded; otherwise it is not read at all (a dst full
// of NaN comes out clean).  NORM: the workgroup's share of sum |stored value|^2 goes to partials[block]; the grid is then
// capped (reduce_grid) and the loop runs more than once from 2^18 amplitudes on.  The sum is formed in the order beta dst,
// c_0 src_0, c_1 src_1, ... whatever the split into passes.  One amplitude per thread and trip: a NORM pass that loaded
// four (two) amplitudes a grid stride apart before using any was measured slower for up to two sources and 2-3 % faster
// for four and eight.
template <int K, bool BETA, bool NORM, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_lincomb(amp_t *__restrict__ dst, const LincombArgs g, double *__restrict__ partials) {
    double norm = 0.0, unused = 0.0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < g.amps; i += stride) {
        amp_t s[K > 0 ? K : 1];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = ld<NT>(static_cast<const amp_t *>(g.src[k]) + i);
        amp_t acc = amp_t{0.0, 0.0};
        if constexpr (BETA) acc = cmul(cplx{g.beta_re, g.beta_im}, ld<NT>(dst + i));
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const cplx c = {g.c_re[k], g.c_im[k]};
            acc = (k == 0 && !BETA) ? cmul(c, s[0]) : cfma(c, s[k], acc);
        }
        st<NT>(dst + i, acc);
        if constexpr (NORM) norm = fma(acc.x, acc.x, fma(acc.y, acc.y, norm));
    }
    if constexpr (NORM) {
        block_sum2(norm, unused);
        if (threadIdx.x == 0) partials[blockIdx.x] = norm;
    }
}

// conj(x) y
__device__ __forceinline__ amp_t conj_mul(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.x, y.y, -(x.y * y.x))};
}

// partials[(block * K + k) * 2 + {0, 1}] = this workgroup's share of <x_k|y> = sum_i conj(x_k[i]) y[i], k < K: y is loaded
// once per amplitude and each x_k once, K complex accumulators per thread.  Wave shuffle, then LDS, then one partial per
// workgroup and slot (the host sums them in index order: deterministic).  Read-only; x_k may be y.
template <int K>
__global__ __launch_bounds__(QSV_BLOCK) void k_inner_many(const amp_t *__restrict__ y, const InnerManyArgs g, double *__restrict__ partials) {
    double re[K], im[K];
#pragma unroll
    for (int k = 0; k < K; ++k) re[k] = im[k] = 0.0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < g.amps; i += stride) {
        const amp_t yv = y[i];
        amp_t x[K];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = static_cast<const amp_t *>(g.x[k])[i];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const amp_t p = conj_mul(x[k], yv);
            re[k] += p.x;
            im[k] += p.y;
        }
    }
    __shared__ double sums[QSV_BLOCK / 64][2 * K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double sr = wave_sum(re[k]), si = wave_sum(im[k]);
        if ((threadIdx.x & 63) == 0) {
            sums[threadIdx.x >> 6][2 * k] = sr;
            sums[threadIdx.x >> 6][2 * k + 1] = si;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        double s = 0.0;
        for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) s += sums[wv][threadIdx.x];
        partials[static_cast<uint64_t>(blockIdx.x) * (2 * K) + threadIdx.x] = s;
    }
}

// [a, a + amps_a) and [b, b + amps_b) amplitudes meet
bool ranges_meet(const amp_t *a, uint64_t amps_a, const amp_t *b, uint64_t amps_b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + sizeof(amp_t) * amps_b && b0 < a0 + sizeof(amp_t) * amps_a;
}

// Every pass of a qsv_lincomb call, back to back on dst's stream; one copy and one synchronisation at the end only where
// the norm is wanted.
int lincomb_passes_launch(qsv_state *dst, uint64_t amps, int n_src, const void *const *srcs, const double *coeffs, double beta_re,
                          double beta_im, double *norm2, uint64_t *passes) {
    const std::vector<LincombPass> plan = lincomb_passes(n_src, beta_re, beta_im, norm2 != nullptr, amps, dst->grid_cap);
    const LincombPass &last = plan.back();
    if (norm2) {
        const int rc = qsvk_ensure_matrix(dst, sizeof(double) * last.grid);
        if (rc) return rc;
    }
    for (const LincombPass &p : plan) {
        const LincombArgs g = lincomb_args(p, amps, coeffs, srcs);
        const bool nt = dst->nontemporal != 0;
        const dim3 gd(p.grid), bd(QSV_BLOCK);
        double *out = p.norm ? dst->dev_matrix + p.partial_offset : nullptr;
        with_int<0, KRYLOV_OPERANDS_PER_PASS>(p.count, [&](auto K) { with_bool(p.reads_dst, [&](auto BETA) { with_bool(p.norm, [&](auto NORM) { with_bool(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_lincomb<K.value, BETA.value, NORM.value, NT.value>), gd, bd, 0, dst->stream, dst->data, g, out);
        }); }); }); });
        snprintf(dst->last_kernel, sizeof(dst->last_kernel), "k_lincomb<%d, %s, %s, %s>", p.count, p.reads_dst ? "true" : "false",
                 p.norm ? "true" : "false", nt ? "true" : "false");
        const int rc = check_launch();
        if (rc) return rc;
    }
    if (passes) *passes = plan.size();
    if (norm2) {
        std::vector<double> host(last.grid);
        QSV_HIP(hipMemcpyAsync(host.data(), dst->dev_matrix + last.partial_offset, sizeof(double) * last.grid, hipMemcpyDeviceToHost, dst->stream));
        QSV_HIP(hipStreamSynchronize(dst->stream));
        double s = 0.0;
        for (int b = 0; b < last.grid; ++b) s += host[b];
        *norm2 = s;
    }
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_lincomb(qsv_state *dst, double beta_re, double beta_im, int n_src, qsv_state *const *srcs, const double *coeffs,
                double *norm2, uint64_t *passes) {
    if (!dst) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_src < 0) return qsv_fail(QSV_EINVAL, "negative number of source registers");
    if (n_src > 0 && (!srcs || !coeffs)) return qsv_fail(QSV_EINVAL, "null pointer");
    for (int k = 0; k < n_src; ++k)
        if (!srcs[k]) return qsv_fail(QSV_EINVAL, "null pointer");
    if (dst->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    for (int k = 0; k < n_src; ++k)
        if (srcs[k]->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    const bool beta = !(beta_re == 0.0 && beta_im == 0.0);
    const uint64_t amps = n_src > 0 ? srcs[0]->amps : dst->amps;
    const int n = n_src > 0 ? srcs[0]->n : dst->n;
    for (int k = 0; k < n_src; ++k) {
        if (srcs[k]->device != dst->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
        if (srcs[k]->n != n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    }
    if (dst->capacity < amps) return qsv_fail(QSV_ENOMEM, "destination register too small");
    if (beta && dst->n != n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    for (int k = 0; k < n_src; ++k)
        if (srcs[k] == dst || ranges_meet(dst->data, amps, srcs[k]->data, amps))
            return qsv_fail(QSV_EINVAL, "the destination must not share memory with a source (fold its coefficient into beta)");
    if (passes) *passes = 0;
    // everything is checked: now the queues, then the streams of the registers that are only read
    int rc = qsv_flush(dst);
    if (rc) return rc;
    for (int k = 0; k < n_src; ++k) {
        rc = qsv_flush(srcs[k]);
        if (rc) return rc;
    }
    QSV_HIP(hipSetDevice(dst->device));
    std::vector<const void *> data(n_src);
    for (int k = 0; k < n_src; ++k) {
        if (srcs[k]->stream != dst->stream) QSV_HIP(hipStreamSynchronize(srcs[k]->stream));
        data[k] = srcs[k]->data;
    }
    rc = lincomb_passes_launch(dst, amps, n_src, data.data(), coeffs, beta_re, beta_im, norm2, passes);
    if (rc) return rc;
    // dst takes the sources' size only once every launch went out, as in qsv_copy
    dst->n = n;
    dst->amps = amps;
    return QSV_OK;
}

int qsv_inner_many(qsv_state *y, int n_x, qsv_state *const *xs, double *values, uint64_t *passes) {
    if (!y) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_x < 0) return qsv_fail(QSV_EINVAL, "negative number of registers");
    if (n_x > 0 && (!xs || !values)) return qsv_fail(QSV_EINVAL, "null pointer");
    for (int k = 0; k < n_x; ++k)
        if (!xs[k]) return qsv_fail(QSV_EINVAL, "null pointer");
    if (y->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    for (int k = 0; k < n_x; ++k)
        if (xs[k]->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    for (int k = 0; k < n_x; ++k) {
        if (xs[k]->device != y->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
        if (xs[k]->n != y->n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    }
    if (passes) *passes = 0;
    if (n_x == 0) return QSV_OK;
    int rc = qsv_flush(y);
    if (rc) return rc;
    for (int k = 0; k < n_x; ++k) {
        rc = qsv_flush(xs[k]);
        if (rc) return rc;
    }
    QSV_HIP(hipSetDevice(y->device));
    std::vector<const void *> data(n_x);
    for (int k = 0; k < n_x; ++k) {
        if (xs[k]->stream != y->stream) QSV_HIP(hipStreamSynchronize(xs[k]->stream));
        data[k] = xs[k]->data;
    }
    const InnerPlan plan = inner_plan(n_x, y->amps, y->grid_cap);
    rc = qsvk_ensure_matrix(y, sizeof(double) * plan.doubles);
    if (rc) return rc;
    for (const InnerPass &p : plan.passes) {
        const InnerManyArgs g = inner_args(p, y->amps, data.data());
        double *out = y->dev_matrix + p.partial_offset;
        with_int<1, KRYLOV_OPERANDS_PER_PASS>(p.count, [&](auto K) {
            hipLaunchKernelGGL((k_inner_many<K.value>), dim3(p.grid), dim3(QSV_BLOCK), 0, y->stream, y->data, g, out);
        });
        snprintf(y->last_kernel, sizeof(y->last_kernel), "k_inner_many<%d>", p.count);
        rc = check_launch();
        if (rc) {
            (void)hipStreamSynchronize(y->stream);
            return rc;
        }
    }
    std::vector<double> host(plan.doubles);
    QSV_HIP(hipMemcpyAsync(host.data(), y->dev_matrix, sizeof(double) * plan.doubles, hipMemcpyDeviceToHost, y->stream));
    QSV_HIP(hipStreamSynchronize(y->stream));
    for (const InnerPass &p : plan.passes) inner_sum(p, host.data(), values);
    if (passes) *passes = plan.passes.size();
    return QSV_OK;
}

}  // extern "C"

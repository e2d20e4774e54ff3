// Pauli-string kernels of the qubit register (gfx950, wave64): expectation values of single strings and of planned
// groups (qsv_pauli_plan.h), planned rotations (qsv_pauli_rotation_plan.h), and Pauli sums as operators (H src into a
// register, <bra|H|ket>, and the backward walk over a rotation list), with their launchers.  The argument structs are
// filled by qsv_readout_layout.h.

#include "qsv_device.h"
#include "qsv_pauli_rotate_item.h"

#include <cstring>
#include <vector>

using namespace qsv_readout_layout;

namespace {

// <psi| P |psi> for a Pauli string: P|i> = i^{nY} (-1)^{popcount(i & zmask)} |i ^ xmask>  (Y = i X Z).
// partials[2b], [2b+1] = real and imaginary part of this block's share of sum_i conj(psi[i ^ xmask]) sign(i) psi[i];
// the factor i^{nY} is applied on the host.
__global__ __launch_bounds__(QSV_BLOCK) void k_expect_pauli(const amp_t *__restrict__ a, uint64_t amps,
                                                           uint64_t xmask, uint64_t zmask,
                                                           double *__restrict__ partials) {
    double re = 0.0, im = 0.0;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const amp_t x = a[i ^ xmask], y = a[i];
        const double s = (__popcll(i & zmask) & 1) ? -1.0 : 1.0;
        re += s * (x.x * y.x + x.y * y.y);  // conj(x) * y
        im += s * (x.x * y.y - x.y * y.x);
    }
    block_sum2(re, im);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = re;
        partials[2 * blockIdx.x + 1] = im;
    }
}

// partials[block * T + t] = this block's share of sum_i s_t(i) Re c(i) (Im c(i) for odd nY) over the visited i:
// every i for the diagonal group (c = |psi[i]|^2), the i with a clear pivot bit otherwise (c = conj(psi[i ^ xmask]) psi[i],
// each amplitude read once).  The product is formed once per item; a term costs a sign and one double accumulator.
// PAULI_ITEMS independent items are loaded before any is used, so a thread keeps 2 x PAULI_ITEMS 16-byte loads in flight.
constexpr int PAULI_ITEMS = 4;

template <int T, bool DIAG>
__global__ __launch_bounds__(QSV_BLOCK) void k_expect_pauli_group(const amp_t *__restrict__ a, const PauliPassArgs g,
                                                                 double *__restrict__ partials) {
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    auto add = [&](uint64_t i, double re, double im) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double v = (!DIAG && ((g.odd >> t) & 1u)) ? im : re;
            acc[t] += (__popcll(i & g.zmask[t]) & 1) ? -v : v;
        }
    };
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    uint64_t w = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    for (; w + (PAULI_ITEMS - 1) * stride < g.items; w += PAULI_ITEMS * stride) {
        uint64_t i[PAULI_ITEMS];
        amp_t x[PAULI_ITEMS], y[PAULI_ITEMS];
#pragma unroll
        for (int u = 0; u < PAULI_ITEMS; ++u) {
            i[u] = DIAG ? w + u * stride : insert_zero(w + u * stride, g.pivot);
            y[u] = a[i[u]];
            if constexpr (!DIAG) x[u] = a[i[u] ^ g.xmask];
        }
#pragma unroll
        for (int u = 0; u < PAULI_ITEMS; ++u) {
            if constexpr (DIAG) add(i[u], y[u].x * y[u].x + y[u].y * y[u].y, 0.0);
            else add(i[u], x[u].x * y[u].x + x[u].y * y[u].y, x[u].x * y[u].y - x[u].y * y[u].x);   // conj(x) * y
        }
    }
    for (; w < g.items; w += stride) {
        const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
        const amp_t y = a[i];
        if constexpr (DIAG) {
            add(i, y.x * y.x + y.y * y.y, 0.0);
        } else {
            const amp_t x = a[i ^ g.xmask];
            add(i, x.x * y.x + x.y * y.y, x.x * y.y - x.y * y.x);
        }
    }
    __shared__ double sums[QSV_BLOCK / 64][T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const double s = wave_sum(acc[t]);
        if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6][t] = s;
    }
    __syncthreads();
    if (threadIdx.x < T) {
        double s = 0.0;
        for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) s += sums[wv][threadIdx.x];
        partials[static_cast<uint64_t>(blockIdx.x) * T + threadIdx.x] = s;
    }
}

// The item body of a rotation pass (pauli_rotate_term, pauli_rotate_item): qsv_pauli_rotate_item.h, shared with qsv_sweep.hip.

// Work item w owns amplitude w (DIAG) or the pair {i, i ^ xmask} with i = insert_zero(w, pivot): it loads it, applies the
// pass in registers and stores it -- in place, no barrier, no LDS.  One work item per thread, as in the gate kernels: a
// pair item has its two 16-byte loads in flight together, and more items per thread were measured slower (DESIGN.md,
// "Pauli rotations").  With the pivot at the highest flipped bit the i of a workgroup are consecutive (up to the one jump
// over the pivot bit) and so are the partners, up to a permutation inside their range: for pivot >= 3 every wave access
// covers whole 128-byte lines.  For a pivot on bits 0..2 the two halves of a line belong to the same thread or to a
// neighbour; these passes use plain (cached) accesses so that the halves meet in L2 before the line is written back
// (NT = false).  The loop only runs more than once beyond 2^32 work items (grid_for).
template <int T, bool DIAG, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_pauli_rotate_group(amp_t *__restrict__ psi, const PauliRotateArgs g) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.items; w += stride) {
        const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
        amp_t a = ld<NT>(psi + i), b = amp_t{0.0, 0.0};
        if constexpr (!DIAG) b = ld<NT>(psi + (i ^ g.xmask));
        pauli_rotate_item<T, DIAG>(g, i, a, b);
        st<NT>(psi + i, a);
        if constexpr (!DIAG) st<NT>(psi + (i ^ g.xmask), b);
    }
}

// dst (+)= (sum_t c_t P_t) src for the T terms of one planned pass of qsv_apply_pauli_sum, all with the pass's xmask.  Work
// item w owns the pair {i, j = i ^ xmask}, i = insert_zero(w, pivot), or amplitude w when DIAG.  With d_t = c_t i^{nY_t}
// (host) and s_t(j) = (-1)^{nY_t} s_t(i):  dst[i] (+)= f_i src[j],  dst[j] (+)= f_j src[i],  f_j = e + o,  f_i = e - o,
// where e (o) sums d_t s_t(i) over the terms with even (odd) nY -- one sign selection per term serves both factors, and
// which sum a term joins is wave-uniform.  FIRST: the first pass of a call that overwrites; the old dst is not read (a
// pair pass and a diagonal pass both cover every amplitude).  Two register streams when FIRST, three otherwise.  Pivot
// and NT as in k_pauli_rotate_group: plain accesses for a pivot on bits 0..2.
template <int T, bool DIAG, bool FIRST, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_pauli_sum_apply_group(amp_t *__restrict__ dst, const amp_t *__restrict__ src,
                                                                    const PauliSumApplyArgs g) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.items; w += stride) {
        const uint64_t i = DIAG ? w : insert_zero(w, g.pivot), j = i ^ g.xmask;
        const amp_t a = ld<NT>(src + i);
        amp_t b = amp_t{0.0, 0.0}, old_i = amp_t{0.0, 0.0}, old_j = amp_t{0.0, 0.0};
        if constexpr (!DIAG) b = ld<NT>(src + j);
        if constexpr (!FIRST) {
            old_i = ld<NT>(dst + i);
            if constexpr (!DIAG) old_j = ld<NT>(dst + j);
        }
        cplx e = {0.0, 0.0}, o = {0.0, 0.0};
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const bool minus = __popcll(i & g.zmask[t]) & 1;
            const double re = minus ? -g.d_re[t] : g.d_re[t], im = minus ? -g.d_im[t] : g.d_im[t];
            if (!DIAG && ((g.odd >> t) & 1u)) {
                o.re += re;
                o.im += im;
            } else {
                e.re += re;
                e.im += im;
            }
        }
        if constexpr (DIAG) {
            st<NT>(dst + i, cfma(e, a, old_i));
        } else {
            st<NT>(dst + i, cfma(cplx{e.re - o.re, e.im - o.im}, b, old_i));
            st<NT>(dst + j, cfma(cplx{e.re + o.re, e.im + o.im}, a, old_j));
        }
    }
}

// conj(x) y
__device__ __forceinline__ amp_t conj_mul(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.x, y.y, -(x.y * y.x))};
}

// Per-term complex accumulators of a workgroup -> partials[(block * T + t) * 2 + {0, 1}]: wave shuffle, then LDS, then
// one partial per workgroup and term (the host sums them in index order: deterministic).
template <int T>
__device__ __forceinline__ void store_term_partials(const double (&re)[T], const double (&im)[T], double *__restrict__ partials) {
    __shared__ double sums[QSV_BLOCK / 64][2 * T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const double sr = wave_sum(re[t]), si = wave_sum(im[t]);
        if ((threadIdx.x & 63) == 0) {
            sums[threadIdx.x >> 6][2 * t] = sr;
            sums[threadIdx.x >> 6][2 * t + 1] = si;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * T) {
        double s = 0.0;
        for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) s += sums[wv][threadIdx.x];
        partials[static_cast<uint64_t>(blockIdx.x) * (2 * T) + threadIdx.x] = s;
    }
}

// <bra| P_t |ket> / i^{nY_t} for the T terms of one planned pass of qsv_pauli_transition_sum.  A work item visits the pair
// {i, j = i ^ xmask} through the i whose pivot bit is clear: with u = conj(bra[i]) ket[j] and v = conj(bra[j]) ket[i] term
// t gets s_t(i) (v + (-1)^{nY_t} u); v + u and v - u are formed once, a term costs a sign and one complex accumulator.
// DIAG: every i, s_t(i) conj(bra[i]) ket[i].  Read-only; the factor i^{nY} is applied on the host.
template <int T, bool DIAG>
__global__ __launch_bounds__(QSV_BLOCK) void k_pauli_transition_group(const amp_t *__restrict__ bra, const amp_t *__restrict__ ket,
                                                                     const PauliPassArgs g, double *__restrict__ partials) {
    double re[T], im[T];
#pragma unroll
    for (int t = 0; t < T; ++t) re[t] = im[t] = 0.0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.items; w += stride) {
        const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
        amp_t even, odd = amp_t{0.0, 0.0};
        if constexpr (DIAG) {
            even = conj_mul(bra[i], ket[i]);
        } else {
            const amp_t bi = bra[i], bj = bra[i ^ g.xmask], ki = ket[i], kj = ket[i ^ g.xmask];
            const amp_t u = conj_mul(bi, kj), v = conj_mul(bj, ki);
            even = v + u;
            odd = v - u;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const amp_t x = (!DIAG && ((g.odd >> t) & 1u)) ? odd : even;
            const bool minus = __popcll(i & g.zmask[t]) & 1;
            re[t] += minus ? -x.x : x.x;
            im[t] += minus ? -x.y : x.y;
        }
    }
    store_term_partials<T>(re, im, partials);
}

// One pass of the backward walk of qsv_pauli_rotations_adjoint.  g holds a pass of the forward plan with its terms in
// reverse order and -theta (pauli_adjoint_args).  A work item loads its pair of psi and its pair of lambda and, slot by
// slot, adds the pair's share of <lambda| P |psi> / i^{nY} to the slot's accumulator --
//     flipping term:  s(i) (v + (-1)^{nY} u),  u = conj(l_i) p_j,  v = conj(l_j) p_i
//     diagonal term:  s(i) conj(l_i) p_i + s(j) conj(l_j) p_j
// -- and then undoes the slot's rotation on both pairs in registers; it stores the four amplitudes at the end.  Padding
// slots (theta = 0, diagonal) leave the data alone and the host ignores their accumulators.  Four register streams per
// pass.  The grid is capped (one partial per workgroup and slot, summed by the host), so the loop does run more than
// once on registers beyond QSV_REDUCE_BLOCKS x QSV_BLOCK work items.  Pivot and NT as in k_pauli_rotate_group.
template <int T, bool DIAG, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_pauli_adjoint_group(amp_t *__restrict__ psi, amp_t *__restrict__ lambda,
                                                                  const PauliRotateArgs g, double *__restrict__ partials) {
    double re[T], im[T];
#pragma unroll
    for (int t = 0; t < T; ++t) re[t] = im[t] = 0.0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.items; w += stride) {
        const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
        amp_t pa = ld<NT>(psi + i), la = ld<NT>(lambda + i), pb = amp_t{0.0, 0.0}, lb = amp_t{0.0, 0.0};
        if constexpr (!DIAG) {
            pb = ld<NT>(psi + (i ^ g.xmask));
            lb = ld<NT>(lambda + (i ^ g.xmask));
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t z = g.zmask[t];
            const bool minus = __popcll(i & z) & 1;
            amp_t x;
            if (DIAG || ((g.diag >> t) & 1u)) {
                x = conj_mul(la, pa);
                if constexpr (!DIAG) {
                    const amp_t y = conj_mul(lb, pb);
                    x = (__popcll(g.xmask & z) & 1) ? x - y : x + y;
                }
            } else {
                const amp_t u = conj_mul(la, pb), v = conj_mul(lb, pa);
                x = ((g.rot >> (2 * t)) & 1u) ? v - u : v + u;
            }
            re[t] += minus ? -x.x : x.x;
            im[t] += minus ? -x.y : x.y;
            pauli_rotate_term<DIAG>(g, t, i, pa, pb);
            pauli_rotate_term<DIAG>(g, t, i, la, lb);
        }
        st<NT>(psi + i, pa);
        st<NT>(lambda + i, la);
        if constexpr (!DIAG) {
            st<NT>(psi + (i ^ g.xmask), pb);
            st<NT>(lambda + (i ^ g.xmask), lb);
        }
    }
    store_term_partials<T>(re, im, partials);
}

}  // namespace

// ----------------------------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------------------------
int qsvk_expect_pauli(qsv_state *st, uint64_t xmask, uint64_t zmask, int n_y, double *re, double *im) {
    const int grid = grid_for(st->amps, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_expect_pauli, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, xmask, zmask,
                       st->partials);
    int rc = check_launch();
    if (rc) return rc;
    double sr = 0.0, si = 0.0;
    rc = sum_partials(st, grid, &sr, &si);
    if (rc) return rc;
    switch (n_y & 3) {  // times i^{nY}
        case 0: *re = sr; *im = si; break;
        case 1: *re = -si; *im = sr; break;
        case 2: *re = -sr; *im = -si; break;
        default: *re = si; *im = -sr; break;
    }
    return QSV_OK;
}

// values[p.index[t]] = <psi|P|psi> of every term of every pass.  The launches go out back to back on the register's
// stream, each with its own slice of the scratch buffer (one partial per workgroup and term); one copy and one
// synchronisation at the end, then the host sums each term's partials in index order (deterministic).
int qsvk_expect_pauli_groups(qsv_state *st, const std::vector<qsv_pauli_plan::Pass> &passes, double *values) {
    if (passes.empty()) return QSV_OK;
    struct Slice { PauliPass pass; size_t offset; int grid; };
    std::vector<Slice> slices;
    size_t doubles = 0;
    for (const qsv_pauli_plan::Pass &p : passes) {
        const PauliPass pass = pauli_pass_args(p, st->amps);
        if (!pass.ok) return qsv_fail(QSV_EINVAL, "bad Pauli pass");
        const int grid = grid_for(pass.g.items, QSV_BLOCK * 2 * PAULI_ITEMS, QSV_REDUCE_BLOCKS);
        slices.push_back({pass, doubles, grid});
        doubles += static_cast<size_t>(grid) * pass.width;
    }
    int rc = qsvk_ensure_matrix(st, sizeof(double) * doubles);
    if (rc) return rc;
    for (size_t k = 0; k < passes.size(); ++k) {
        const Slice &s = slices[k];
        double *out = st->dev_matrix + s.offset;
        with_pow2<1, 8>(s.pass.width, [&](auto W) { with_bool(passes[k].pivot < 0, [&](auto DIAG) {
            hipLaunchKernelGGL((k_expect_pauli_group<W.value, DIAG.value>), dim3(s.grid), dim3(QSV_BLOCK), 0, st->stream, st->data, s.pass.g, out);
        }); });
        rc = check_launch();
        if (rc) {
            (void)hipStreamSynchronize(st->stream);
            return rc;
        }
    }
    std::vector<double> host(doubles);
    QSV_HIP(hipMemcpyAsync(host.data(), st->dev_matrix, sizeof(double) * doubles, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    for (size_t k = 0; k < passes.size(); ++k) {
        const qsv_pauli_plan::Pass &p = passes[k];
        const Slice &s = slices[k];
        for (size_t t = 0; t < p.zmask.size(); ++t) {
            double sum = 0.0;
            for (int b = 0; b < s.grid; ++b) sum += host[s.offset + static_cast<size_t>(b) * s.pass.width + t];
            values[p.index[t]] = qsv_pauli_plan::pair_scale(p.pivot, p.n_y[t]) * sum;
        }
    }
    return QSV_OK;
}

// Every pass of a qsv_apply_pauli_rotations plan, back to back on the register's stream with no host synchronisation.
// cs / sn: cos(theta/2) and sin(theta/2) of every term, indexed as the caller's list.
int qsvk_pauli_rotate_passes(qsv_state *st, const std::vector<qsv_pauli_rotation_plan::Pass> &passes, const double *cs,
                             const double *sn) {
    for (const qsv_pauli_rotation_plan::Pass &p : passes) {
        const PauliRotate r = pauli_rotate_args(p, st->amps, cs, sn);
        if (!r.ok) return qsv_fail(QSV_EINVAL, "bad Pauli rotation pass");
        const bool diag = p.pivot < 0;
        // a pivot inside a 128-byte line: both halves of a line are written by one launch, let them meet in L2
        const bool nt = st->nontemporal && (diag || p.pivot >= 3);
        const dim3 gd(grid_for(r.g.items, QSV_BLOCK, st->grid_cap)), bd(QSV_BLOCK);
        with_pow2<1, 8>(r.width, [&](auto W) { with_bool(diag, [&](auto DIAG) { with_bool(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_pauli_rotate_group<W.value, DIAG.value, NT.value>), gd, bd, 0, st->stream, st->data, r.g);
        }); }); });
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_pauli_rotate_group<%d, %s, %s>", r.width, diag ? "true" : "false",
                 nt ? "true" : "false");
        const int rc = check_launch();
        if (rc) return rc;
    }
    return QSV_OK;
}

// Every pass of a qsv_apply_pauli_sum plan, back to back on dst's stream with no host synchronisation.  amps: src's
// size, which the caller gives dst once every launch went out; coeffs: the interleaved complex coefficient of every term
// of the caller's list.
int qsvk_pauli_sum_apply_passes(qsv_state *dst, const amp_t *src, uint64_t amps, const std::vector<qsv_pauli_plan::Pass> &passes,
                                const double *coeffs, bool accumulate) {
    const std::vector<PauliSumApply> launches = pauli_sum_apply_passes(passes, amps, coeffs, accumulate);
    for (const PauliSumApply &a : launches)
        if (!a.ok) return qsv_fail(QSV_EINVAL, "bad Pauli pass");
    for (const PauliSumApply &a : launches) {
        const bool diag = a.g.xmask == 0;
        const bool nt = dst->nontemporal && (diag || a.g.pivot >= 3);
        const dim3 gd(grid_for(a.g.items, QSV_BLOCK, dst->grid_cap)), bd(QSV_BLOCK);
        with_pow2<1, 8>(a.width, [&](auto W) { with_bool(diag, [&](auto DIAG) { with_bool(a.first, [&](auto FIRST) { with_bool(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_pauli_sum_apply_group<W.value, DIAG.value, FIRST.value, NT.value>), gd, bd, 0, dst->stream, dst->data, src, a.g);
        }); }); }); });
        snprintf(dst->last_kernel, sizeof(dst->last_kernel), "k_pauli_sum_apply_group<%d, %s, %s, %s>", a.width, diag ? "true" : "false",
                 a.first ? "true" : "false", nt ? "true" : "false");
        const int rc = check_launch();
        if (rc) return rc;
    }
    return QSV_OK;
}

// values[2 index, 2 index + 1] = <bra|P|ket> of every term of every pass; launches, slices, copy and host sums as in
// qsvk_expect_pauli_groups, on bra's stream and in bra's scratch buffer.
int qsvk_pauli_transition_groups(qsv_state *bra, const amp_t *ket, const std::vector<qsv_pauli_plan::Pass> &passes, double *values) {
    if (passes.empty()) return QSV_OK;
    struct Slice { PauliPass pass; size_t offset; int grid; };
    std::vector<Slice> slices;
    size_t doubles = 0;
    for (const qsv_pauli_plan::Pass &p : passes) {
        const PauliPass pass = pauli_pass_args(p, bra->amps);
        if (!pass.ok) return qsv_fail(QSV_EINVAL, "bad Pauli pass");
        const int grid = grid_for(pass.g.items, QSV_BLOCK, QSV_REDUCE_BLOCKS);
        slices.push_back({pass, doubles, grid});
        doubles += static_cast<size_t>(grid) * pass.width * 2;
    }
    int rc = qsvk_ensure_matrix(bra, sizeof(double) * doubles);
    if (rc) return rc;
    for (size_t k = 0; k < passes.size(); ++k) {
        const Slice &s = slices[k];
        double *out = bra->dev_matrix + s.offset;
        with_pow2<1, 8>(s.pass.width, [&](auto W) { with_bool(passes[k].pivot < 0, [&](auto DIAG) {
            hipLaunchKernelGGL((k_pauli_transition_group<W.value, DIAG.value>), dim3(s.grid), dim3(QSV_BLOCK), 0, bra->stream, bra->data, ket, s.pass.g, out);
        }); });
        rc = check_launch();
        if (rc) {
            (void)hipStreamSynchronize(bra->stream);
            return rc;
        }
    }
    std::vector<double> host(doubles);
    QSV_HIP(hipMemcpyAsync(host.data(), bra->dev_matrix, sizeof(double) * doubles, hipMemcpyDeviceToHost, bra->stream));
    QSV_HIP(hipStreamSynchronize(bra->stream));
    for (size_t k = 0; k < passes.size(); ++k) {
        const qsv_pauli_plan::Pass &p = passes[k];
        const Slice &s = slices[k];
        for (size_t t = 0; t < p.zmask.size(); ++t) {
            double sr = 0.0, si = 0.0;
            for (int b = 0; b < s.grid; ++b) {
                sr += host[s.offset + (static_cast<size_t>(b) * s.pass.width + t) * 2];
                si += host[s.offset + (static_cast<size_t>(b) * s.pass.width + t) * 2 + 1];
            }
            times_i_pow(p.n_y[t], sr, si, &values[2 * p.index[t]], &values[2 * p.index[t] + 1]);
        }
    }
    return QSV_OK;
}

// The backward walk over a qsv_apply_pauli_rotations plan: its passes last first on psi's stream, with no host
// synchronisation between them.  Every pass writes one partial per workgroup and slot into its own slice of psi's scratch
// buffer; a chunk of passes ends with one copy and one synchronisation.  A chunk holds as many passes as fit
// PAULI_ADJOINT_SCRATCH doubles (1 MiB: at least 8 passes of 8 rotations on a full grid of QSV_REDUCE_BLOCKS workgroups, so
// a list of 100 rotations costs at most 4 synchronisations on a large register and one on a small one).
// values[2 index, 2 index + 1] = <lambda|P|psi> at the moment the walk reaches the term.
constexpr size_t PAULI_ADJOINT_SCRATCH = (1u << 20) / sizeof(double);

int qsvk_pauli_adjoint_passes(qsv_state *psi, amp_t *lambda, const std::vector<qsv_pauli_rotation_plan::Pass> &passes,
                              const double *cs, const double *sn, double *values) {
    const std::vector<PauliAdjoint> walk = pauli_adjoint_passes(passes, psi->amps, cs, sn);
    for (const PauliAdjoint &a : walk)
        if (!a.r.ok) return qsv_fail(QSV_EINVAL, "bad Pauli rotation pass");
    std::vector<double> host;
    for (size_t first = 0; first < walk.size();) {
        std::vector<size_t> offset;
        std::vector<int> grids;
        size_t doubles = 0, last = first;
        for (; last < walk.size(); ++last) {
            const int grid = grid_for(walk[last].r.g.items, QSV_BLOCK, QSV_REDUCE_BLOCKS);
            const size_t need = static_cast<size_t>(grid) * walk[last].r.width * 2;
            if (last > first && doubles + need > PAULI_ADJOINT_SCRATCH) break;
            offset.push_back(doubles);
            grids.push_back(grid);
            doubles += need;
        }
        int rc = qsvk_ensure_matrix(psi, sizeof(double) * doubles);
        if (rc) return rc;
        for (size_t k = first; k < last; ++k) {
            const PauliRotate &r = walk[k].r;
            const bool diag = r.g.xmask == 0;
            const bool nt = psi->nontemporal && (diag || r.g.pivot >= 3);
            double *out = psi->dev_matrix + offset[k - first];
            with_pow2<1, 8>(r.width, [&](auto W) { with_bool(diag, [&](auto DIAG) { with_bool(nt, [&](auto NT) {
                hipLaunchKernelGGL((k_pauli_adjoint_group<W.value, DIAG.value, NT.value>), dim3(grids[k - first]), dim3(QSV_BLOCK), 0, psi->stream,
                                   psi->data, lambda, r.g, out);
            }); }); });
            snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_pauli_adjoint_group<%d, %s, %s>", r.width, diag ? "true" : "false",
                     nt ? "true" : "false");
            rc = check_launch();
            if (rc) {
                (void)hipStreamSynchronize(psi->stream);
                return rc;
            }
        }
        host.resize(doubles);
        QSV_HIP(hipMemcpyAsync(host.data(), psi->dev_matrix, sizeof(double) * doubles, hipMemcpyDeviceToHost, psi->stream));
        QSV_HIP(hipStreamSynchronize(psi->stream));
        for (size_t k = first; k < last; ++k) {
            const PauliAdjoint &a = walk[k];
            for (int t = 0; t < qsv_pauli_rotation_plan::ROTATIONS_PER_PASS && a.index[t] >= 0; ++t) {
                double sr = 0.0, si = 0.0;
                for (int b = 0; b < grids[k - first]; ++b) {
                    sr += host[offset[k - first] + (static_cast<size_t>(b) * a.r.width + t) * 2];
                    si += host[offset[k - first] + (static_cast<size_t>(b) * a.r.width + t) * 2 + 1];
                }
                times_i_pow(a.n_y[t], sr, si, &values[2 * a.index[t]], &values[2 * a.index[t] + 1]);
            }
        }
        first = last;
    }
    return QSV_OK;
}

// Pauli-string kernels of the qubit register (gfx950, wave64): expectation values of single strings and of planned
// groups (qsv_pauli_plan.h), and planned rotations (qsv_pauli_rotation_plan.h), with their launchers.  The argument
// structs are filled by qsv_readout_layout.h.

#include "qsv_device.h"

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

// i^k v: a swap and signs of the real and imaginary part, never a multiplication (k is wave-uniform)
__device__ __forceinline__ amp_t mul_i_pow(amp_t v, uint32_t k) {
    amp_t r;
    r.x = (k & 1u) ? v.y : v.x;
    r.y = (k & 1u) ? v.x : v.y;
    if (k == 1u || k == 2u) r.x = -r.x;
    if (k >= 2u) r.y = -r.y;
    return r;
}

// (c - i t) v
__device__ __forceinline__ amp_t phase_amp(double c, double t, amp_t v) {
    amp_t r;
    r.x = fma(t, v.y, c * v.x);
    r.y = fma(-t, v.x, c * v.y);
    return r;
}

// The T terms of the pass on one work item, in the caller's order.  a = psi[i], b = psi[i ^ xmask] (unused when DIAG);
// s(j) = (-1)^{popcount(j & zmask)} and s(i ^ xmask) = s(i) s(xmask).  What a term is (diagonal or not, its power of i,
// whether its sign differs between the partners) is wave-uniform: scalar branches, no divergence.
template <int T, bool DIAG>
__device__ __forceinline__ void pauli_rotate_item(const PauliRotateArgs &g, uint64_t i, amp_t &a, amp_t &b) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t z = g.zmask[t];
        const double c = g.cs[t], sn = g.sn[t];
        const bool minus = __popcll(i & z) & 1;                   // s(i) = -1
        if (DIAG || ((g.diag >> t) & 1u)) {
            a = phase_amp(c, minus ? -sn : sn, a);
            if constexpr (!DIAG) {
                const bool differ = __popcll(g.xmask & z) & 1;
                b = phase_amp(c, (minus != differ) ? -sn : sn, b);
            }
        } else if constexpr (!DIAG) {
            const uint32_t n_y = (g.rot >> (2 * t)) & 3u, k = (n_y + 3u) & 3u;   // -i i^{nY} = i^k
            const bool differ = n_y & 1u;                                       // s(i') = (-1)^{nY} s(i)
            const double ta = (minus != differ) ? -sn : sn;   // sn s(i'), in front of b in a'
            const double tb = minus ? -sn : sn;               // sn s(i),  in front of a in b'
            const amp_t ra = mul_i_pow(a, k), rb = mul_i_pow(b, k);
            a = amp_t{fma(ta, rb.x, c * a.x), fma(ta, rb.y, c * a.y)};
            b = amp_t{fma(tb, ra.x, c * b.x), fma(tb, ra.y, c * b.y)};
        }
    }
}

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

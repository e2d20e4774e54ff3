// Per-member adjoint walks (gfx950, wave64): every member of an ensemble (qsv_ensemble_layout.h) runs the
// backward walk of qsv_pauli_rotations_adjoint and of qsv_diag_phase_adjoint with its own angles, and reads back its own
// <lambda_m|P_t|psi_m>, <lambda_m|D|psi_m> and <a_m|b_m>.
//   k_ens_pauli_adjoint_group  k_pauli_adjoint_group's item body on member-local items, -theta from the device table of
//                              qsv_sweep_layout.h read in the walk's order, ended by member_store_sums<2 T>;
//   k_ens_adjoint_sum          a pass's partials summed part by part into results[member][term][re, im];
//   k_ens_diag_phase_adjoint   k_diag_phase_adjoint with the member's gamma and the diagonal indexed by the member-local index;
//   k_ens_inner                <a_m|b_m> on the units of a read pass;
//   k_ens_diag_mul             lambda_m = D psi_m, k_diag_mul with the diagonal indexed by the member-local index.
// The per-item arithmetic is the single-register kernels' own (qsv_pauli_rotate_item.h, qsv_diagonal_device.h): a member's
// registers round exactly as registers of their own would.  Launch shapes: qsv_sweep_layout.h.

#include "qsv_device.h"
#include "qsv_diagonal_device.h"
#include "qsv_ensemble_device.h"
#include "qsv_pauli_rotate_item.h"
#include "qsv_sweep_layout.h"

#include <cmath>
#include <vector>

using namespace qsv_ensemble_layout;
using namespace qsv_sweep_layout;
using qsv_readout_layout::pauli_adjoint_args;
using qsv_readout_layout::PauliAdjoint;
using qsv_readout_layout::PauliRotateArgs;
using qsv_readout_layout::times_i_pow;

namespace {

// conj(x) y, as k_pauli_adjoint_group and k_diag_phase_adjoint form it
__device__ __forceinline__ amp_t conj_mul(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.x, y.y, -(x.y * y.x))};
}

// k_pauli_adjoint_group's item body on the items of one member (k_ens_pauli_rotate_group's index arithmetic): g holds a pass
// of the forward plan with its terms in reverse order (pauli_adjoint_args); slot k < s.count takes cos, -sin of term
// s.count - 1 - k of the pass from the member's row of the table, the slots beyond the count the padding theta = 0.  The
// row is fetched once per unit, all T slots without a branch (TABLE_PAD).  Every thread of the workgroup reaches
// member_store_sums in every unit: the threads of a member >= members (last shared unit of a small ensemble) fetch the last
// member's row instead of one beyond the table, touch no amplitude and contribute zeros.  WAVE: as in
// k_ens_pauli_rotate_group, the fetch is a scalar load where a wave lies in one member.
template <int T, bool DIAG, bool NT, bool WAVE>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_pauli_adjoint_group(amp_t *__restrict__ psi, amp_t *__restrict__ lambda, const PauliRotateArgs g,
                                                                       const EnsArgs e, const SweepArgs s, const double *__restrict__ table,
                                                                       double *__restrict__ partials) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        const uint64_t clamped = t.live ? t.member : e.members - 1;     // for the fetch and the addresses only
        const uint64_t member = WAVE ? wave_uniform(clamped) : clamped;
        const double *row = table + member * s.row_doubles + s.first;
        PauliRotateArgs h = g;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int at = k < s.count ? s.count - 1 - k : k;
            const double c = row[2 * at], sn = row[2 * at + 1];
            h.cs[k] = k < s.count ? c : 1.0;
            h.sn[k] = k < s.count ? sn : 0.0;
        }
        double v[2 * T];
#pragma unroll
        for (int k = 0; k < 2 * T; ++k) v[k] = 0.0;
        if (t.live) {
            amp_t *pm = psi + (member << e.n), *lm = lambda + (member << e.n);
            for (uint64_t w = t.first; w < t.items; w += t.stride) {
                const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
                amp_t pa = ld<NT>(pm + i), la = ld<NT>(lm + i), pb = amp_t{0.0, 0.0}, lb = amp_t{0.0, 0.0};
                if constexpr (!DIAG) {
                    pb = ld<NT>(pm + (i ^ g.xmask));
                    lb = ld<NT>(lm + (i ^ g.xmask));
                }
#pragma unroll
                for (int k = 0; k < T; ++k) {
                    const uint64_t z = h.zmask[k];
                    const bool minus = __popcll(i & z) & 1;
                    amp_t x;
                    if (DIAG || ((h.diag >> k) & 1u)) {
                        x = conj_mul(la, pa);
                        if constexpr (!DIAG) {
                            const amp_t y = conj_mul(lb, pb);
                            x = (__popcll(h.xmask & z) & 1) ? x - y : x + y;
                        }
                    } else {
                        const amp_t u = conj_mul(la, pb), vv = conj_mul(lb, pa);
                        x = ((h.rot >> (2 * k)) & 1u) ? vv - u : vv + u;
                    }
                    v[2 * k] += minus ? -x.x : x.x;
                    v[2 * k + 1] += minus ? -x.y : x.y;
                    pauli_rotate_term<DIAG>(h, k, i, pa, pb);
                    pauli_rotate_term<DIAG>(h, k, i, la, lb);
                }
                st<NT>(pm + i, pa);
                st<NT>(lm + i, la);
                if constexpr (!DIAG) {
                    st<NT>(pm + (i ^ g.xmask), pb);
                    st<NT>(lm + (i ^ g.xmask), lb);
                }
            }
        }
        member_store_sums<2 * T>(v, e, t, partials);
    }
}

// results[(member * n_terms + index[t]) * 2 + c] = the sum over the member's parts, in index order, of slot t's re (c = 0) or
// im (c = 1): one thread per (member, slot, c).  Padding slots (index -1) are skipped.
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_adjoint_sum(const double *__restrict__ partials, uint64_t members, const AdjointSumArgs a,
                                                               double *__restrict__ results) {
    const uint64_t R = 2 * static_cast<uint64_t>(a.width), count = members * R, stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < count; i += stride) {
        const uint64_t m = i / R;
        const int r = static_cast<int>(i % R);
        const int index = a.index[r >> 1];
        if (index < 0) continue;
        const double *p = partials + m * a.parts * R + r;
        double sum = 0.0;
        for (int q = 0; q < a.parts; ++q) sum += p[static_cast<size_t>(q) * R];
        results[(m * a.n_terms + index) * 2 + (r & 1)] = sum;
    }
}

// k_diag_phase_adjoint per member: partials[member][part][2] = the part's share of <lambda_m|D psi_m>, then both registers
// take exp(-i gammas[m] d): one sincos per amplitude serves both.  The diagonal is read once per member through the caches.
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_diag_phase_adjoint(amp_t *__restrict__ psi, amp_t *__restrict__ lambda, const double *__restrict__ d,
                                                                      const double *__restrict__ gammas, const EnsArgs e, double *__restrict__ partials) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        double v[SWEEP_PAIR_SLOTS] = {0.0, 0.0};
        if (t.live) {
            const double gamma = gammas[t.member];
            amp_t *pm = psi + (t.member << e.n), *lm = lambda + (t.member << e.n);
            for (uint64_t w = t.first; w < t.items; w += t.stride) {
                const amp_t a = ld<NT>(pm + w), l = ld<NT>(lm + w);
                const double x = d[w];
                const amp_t p = conj_mul(l, a);
                v[0] = fma(p.x, x, v[0]);
                v[1] = fma(p.y, x, v[1]);
                const cplx ph = phase_of(gamma, x);
                st<NT>(pm + w, cmul(ph, a));
                st<NT>(lm + w, cmul(ph, l));
            }
        }
        member_store_sums<SWEEP_PAIR_SLOTS>(v, e, t, partials);
    }
}

// Im conj(x) y with its two products rounded one by one (no contraction into an fma): exactly 0 for x = y
__device__ __forceinline__ double conj_mul_im(amp_t x, amp_t y) {
#pragma clang fp contract(off)
    const double p = x.x * y.y, q = x.y * y.x;
    return p - q;
}

// partials[member][part][2] = the part's share of <a_m|b_m>.  Read-only; a may be b: <a_m|a_m> has an imaginary part of
// exactly 0 (conj_mul_im).
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_inner(const amp_t *a, const amp_t *b, const EnsArgs e, double *__restrict__ partials) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        double v[SWEEP_PAIR_SLOTS] = {0.0, 0.0};
        if (t.live) {
            const amp_t *am = a + (t.member << e.n), *bm = b + (t.member << e.n);
            for (uint64_t w = t.first; w < t.items; w += t.stride) {
                const amp_t x = am[w], y = bm[w];
                v[0] += fma(x.x, y.x, x.y * y.y);
                v[1] += conj_mul_im(x, y);
            }
        }
        member_store_sums<SWEEP_PAIR_SLOTS>(v, e, t, partials);
    }
}

// dst_m[i] = d[i] src_m[i]: k_diag_mul with the coefficient 1 (its own expressions) and the diagonal indexed by the
// member-local index; a flat loop over the register as k_ens_diag_phase.  dst may be src.
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_diag_mul(amp_t *dst, const amp_t *src, const double *__restrict__ d, uint64_t amps, int n) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK, mask = (1ull << n) - 1ull;
    for (uint64_t idx = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; idx < amps; idx += stride) {
        const amp_t s = ld<NT>(src + idx);
        const double x = d[idx & mask];
        const cplx m = {1.0 * x, 0.0 * x};
        st<NT>(dst + idx, cmul(m, s));
    }
}

bool all_finite(const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// What the three calls refuse about their two registers: each an ensemble register of its own (check_ensemble), of one size
// on one device.  apart: their memory must not meet.
int check_ensemble_pair(const qsv_state *a, const qsv_state *b, int member_qubits, bool apart) {
    int rc = check_ensemble(a, member_qubits, 0);
    if (rc) return rc;
    rc = check_ensemble(b, member_qubits, 0);
    if (rc) return rc;
    if (a->device != b->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    if (a->n != b->n || a->amps != b->amps) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    if (apart) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a->data), b0 = reinterpret_cast<uintptr_t>(b->data);
        const uintptr_t bytes = sizeof(amp_t) * a->amps;
        if (a == b || (a0 < b0 + bytes && b0 < a0 + bytes)) return qsv_fail(QSV_EINVAL, "psi and lambda must be two registers whose memory does not meet");
    }
    return QSV_OK;
}

int check_member_diag(const qsv_state *st, int member_qubits, const qsv_diag *d) {
    if (st->device != d->device) return qsv_fail(QSV_EINVAL, "register and diagonal on different devices");
    if (d->n != member_qubits || d->size != (1ull << member_qubits))
        return qsv_fail(QSV_EINVAL, "the diagonal must have the size of a member (" + std::to_string(member_qubits) + " qubits), not " + std::to_string(d->n));
    return QSV_OK;
}

// both deferred queues, then the other register's stream: the launches go on `first`'s
int flush_pair(qsv_state *first, qsv_state *second) {
    int rc = qsv_flush(first);
    if (rc) return rc;
    if (second != first) {
        rc = qsv_flush(second);
        if (rc) return rc;
    }
    QSV_HIP(hipSetDevice(first->device));
    if (second->stream != first->stream) QSV_HIP(hipStreamSynchronize(second->stream));
    return QSV_OK;
}

// partials [members][parts][2] -> slots [members][2] -> values: one copy and one synchronisation
int fetch_pair_sums(qsv_state *st, const EnsArgs &e, const double *partials, double *slots, double *values) {
    int rc = qsvk_ens_sum_parts(st, partials, e.members, 1 << e.part_bits, SWEEP_PAIR_SLOTS, slots);
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(values, slots, sizeof(double) * pair_values(e.members), hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_ensemble_inner(qsv_state *a, qsv_state *b, int member_qubits, double *values) {
    if (!a || !b || !values) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble_pair(a, b, member_qubits, false);
    if (rc) return rc;
    rc = qsvk_ens_check_member_size(a, member_qubits);
    if (rc) return rc;
    rc = flush_pair(a, b);
    if (rc) return rc;
    double *partials = nullptr, *slots = nullptr;
    rc = qsvk_ens_workspace(a, member_qubits, &partials, &slots);
    if (rc) return rc;
    const EnsArgs e = pair_args(member_qubits, a->amps >> member_qubits, a->grid_cap);
    hipLaunchKernelGGL(k_ens_inner, dim3(ens_grid(e, a->grid_cap)), dim3(QSV_BLOCK), 0, a->stream, static_cast<const amp_t *>(a->data),
                       static_cast<const amp_t *>(b->data), e, partials);
    snprintf(a->last_kernel, sizeof(a->last_kernel), "k_ens_inner");
    rc = check_launch();
    if (rc) return rc;
    return fetch_pair_sums(a, e, partials, slots, values);
}

int qsv_ensemble_apply_diag_mul(qsv_state *dst, qsv_state *src, int member_qubits, qsv_diag *d) {
    if (!dst || !src || !d) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble_pair(src, dst, member_qubits, dst != src);
    if (rc) return rc;
    rc = check_member_diag(src, member_qubits, d);
    if (rc) return rc;
    rc = flush_pair(dst, src);
    if (rc) return rc;
    rc = wait_for_diag(d, dst->stream);
    if (rc) return rc;
    const bool nt = dst->nontemporal != 0;
    with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_ens_diag_mul<NT.value>), dim3(qsv_diagonal_layout::stream_grid(src->amps, dst->grid_cap)), dim3(QSV_BLOCK), 0, dst->stream,
                           dst->data, static_cast<const amp_t *>(src->data), static_cast<const double *>(d->data), src->amps, member_qubits);
    });
    snprintf(dst->last_kernel, sizeof(dst->last_kernel), "k_ens_diag_mul<%s>", nt ? "true" : "false");
    return check_launch();
}

int qsv_ensemble_pauli_rotations_adjoint(qsv_state *psi, qsv_state *lambda, int member_qubits, int n_terms, const int *term_offsets, const int *qubits,
                                         const char *paulis, const double *thetas, double *values, uint64_t *passes) {
    if (!psi || !lambda) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_terms < 0) return qsv_fail(QSV_EINVAL, "negative number of Pauli terms");
    if (n_terms > 0 && (!term_offsets || !thetas || !values)) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble_pair(psi, lambda, member_qubits, true);
    if (rc) return rc;
    // the whole list is checked and turned into masks of member bits before a queue is flushed or anything is launched
    const int n = member_qubits;
    std::vector<qsv_pauli_plan::Term> terms;
    rc = parse_member_terms(n, n_terms, term_offsets, qubits, paulis, &terms);
    if (rc) return rc;
    const uint64_t members = psi->amps >> n;
    if (n_terms > 0 && !all_finite(thetas, static_cast<size_t>(members) * n_terms)) return qsv_fail(QSV_EINVAL, "every angle must be finite");
    rc = qsvk_ens_check_member_size(psi, n);
    if (rc) return rc;
    if (passes) *passes = 0;
    if (n_terms == 0) return QSV_OK;
    // the walk: the forward plan's passes last first, each with its terms in reverse order; masks on a register of one member
    const std::vector<qsv_pauli_rotation_plan::Pass> plan = qsv_pauli_rotation_plan::plan(terms);
    const std::vector<double> ones(static_cast<size_t>(n_terms), 1.0), zeros(static_cast<size_t>(n_terms), 0.0);
    struct Launch { PauliAdjoint a; EnsArgs e; SweepArgs s; bool diag; };
    std::vector<Launch> walk;
    for (size_t k = plan.size(); k-- > 0;) {
        const qsv_pauli_rotation_plan::Pass &p = plan[k];
        Launch l;
        l.a = pauli_adjoint_args(p, 1ull << n, ones.data(), zeros.data());
        if (!l.a.r.ok) return qsv_fail(QSV_EINVAL, "bad Pauli rotation pass");
        l.diag = p.pivot < 0;
        l.e = adjoint_args(n, members, l.diag, psi->grid_cap);
        l.s = sweep_args(n_terms, p.index.front(), static_cast<int>(p.index.size()));
        // a pass's terms are consecutive in the caller's list: the table row is read by position
        for (size_t t = 0; t < p.index.size(); ++t)
            if (p.index[t] != p.index.front() + static_cast<int>(t)) return qsv_fail(QSV_EINVAL, "bad Pauli rotation pass");
        if (!adjoint_fits_workspace(l.e, l.a.r.width)) return qsv_fail(QSV_EINVAL, "the partial sums of a pass do not fit the ensemble workspace");
        walk.push_back(l);
    }
    rc = flush_pair(psi, lambda);
    if (rc) return rc;
    double *partials = nullptr, *slots = nullptr;
    rc = qsvk_ens_workspace(psi, n, &partials, &slots);
    if (rc) return rc;
    // cos, sin of -theta / 2 with the expressions of qsv_pauli_rotations_adjoint (cos kept, sin negated), one row per member;
    // the results [members][n_terms][2] follow the table: everything is sized before the first launch
    const size_t doubles = adjoint_scratch_doubles(members, n_terms);
    std::vector<double> host(table_doubles(members, n_terms), 0.0);
    for (size_t i = 0; i < static_cast<size_t>(members) * n_terms; ++i) {
        host[2 * i] = std::cos(0.5 * thetas[i]);
        host[2 * i + 1] = -std::sin(0.5 * thetas[i]);
    }
    rc = qsvk_ensure_matrix(psi, sizeof(double) * doubles);
    if (rc) return rc;
    double *results = psi->dev_matrix + adjoint_results_offset(members, n_terms);
    // pageable memory: the copy has left `host` when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(psi->dev_matrix, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, psi->stream));
    std::vector<int> n_y(static_cast<size_t>(n_terms), 0);
    for (const Launch &l : walk) {
        const PauliRotateArgs &g = l.a.r.g;
        const int width = l.a.r.width;
        const bool nt = rotate_nontemporal(psi->nontemporal != 0, l.diag, g.pivot);
        const bool wave = wave_in_one_member(l.e);
        const dim3 gd(ens_grid(l.e, psi->grid_cap)), bd(QSV_BLOCK);
        with_pow2<1, 8>(width, [&](auto W) { with_bool(l.diag, [&](auto DIAG) { with_bool(nt, [&](auto NT) { with_bool(wave, [&](auto WAVE) {
            hipLaunchKernelGGL((k_ens_pauli_adjoint_group<W.value, DIAG.value, NT.value, WAVE.value>), gd, bd, 0, psi->stream, psi->data, lambda->data, g,
                               l.e, l.s, static_cast<const double *>(psi->dev_matrix), partials);
        }); }); }); });
        snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_ens_pauli_adjoint_group<%d, %s, %s, %s>", width, l.diag ? "true" : "false",
                 nt ? "true" : "false", wave ? "true" : "false");
        rc = check_launch();
        if (rc) {
            (void)hipStreamSynchronize(psi->stream);
            return rc;
        }
        AdjointSumArgs sum;
        for (int t = 0; t < SWEEP_MAX_SLOTS; ++t) {
            sum.index[t] = t < width ? l.a.index[t] : -1;
            if (l.a.index[t] >= 0) n_y[l.a.index[t]] = l.a.n_y[t];
        }
        sum.width = width;
        sum.parts = 1 << l.e.part_bits;
        sum.n_terms = n_terms;
        sum.pad = 0;
        hipLaunchKernelGGL(k_ens_adjoint_sum, dim3(grid_for(members * 2 * width, QSV_BLOCK, QSV_REDUCE_BLOCKS)), dim3(QSV_BLOCK), 0, psi->stream,
                           static_cast<const double *>(partials), members, sum, results);
        rc = check_launch();
        if (rc) {
            (void)hipStreamSynchronize(psi->stream);
            return rc;
        }
    }
    // one copy and one synchronisation, whatever the list length; then i^{nY} as the single-register call applies it
    std::vector<double> raw(adjoint_results_doubles(members, n_terms));
    QSV_HIP(hipMemcpyAsync(raw.data(), results, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, psi->stream));
    QSV_HIP(hipStreamSynchronize(psi->stream));
    for (uint64_t m = 0; m < members; ++m)
        for (int t = 0; t < n_terms; ++t) {
            const size_t at = 2 * (static_cast<size_t>(m) * n_terms + t);
            times_i_pow(n_y[t], raw[at], raw[at + 1], &values[at], &values[at + 1]);
        }
    if (passes) *passes = plan.size();
    return QSV_OK;
}

int qsv_ensemble_diag_phase_adjoint(qsv_state *psi, qsv_state *lambda, int member_qubits, qsv_diag *d, const double *gammas, double *values) {
    if (!psi || !lambda || !d || !gammas || !values) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble_pair(psi, lambda, member_qubits, true);
    if (rc) return rc;
    rc = check_member_diag(psi, member_qubits, d);
    if (rc) return rc;
    const uint64_t members = psi->amps >> member_qubits;
    if (!all_finite(gammas, members)) return qsv_fail(QSV_EINVAL, "every gamma must be finite");
    rc = qsvk_ens_check_member_size(psi, member_qubits);
    if (rc) return rc;
    rc = flush_pair(psi, lambda);
    if (rc) return rc;
    rc = wait_for_diag(d, psi->stream);
    if (rc) return rc;
    double *partials = nullptr, *slots = nullptr;
    rc = qsvk_ens_workspace(psi, member_qubits, &partials, &slots);
    if (rc) return rc;
    rc = qsvk_ensure_matrix(psi, sizeof(double) * members);
    if (rc) return rc;
    // pageable memory: the copy has left the caller's array when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(psi->dev_matrix, gammas, sizeof(double) * members, hipMemcpyHostToDevice, psi->stream));
    const EnsArgs e = pair_args(member_qubits, members, psi->grid_cap);
    const bool nt = psi->nontemporal != 0;
    with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_ens_diag_phase_adjoint<NT.value>), dim3(ens_grid(e, psi->grid_cap)), dim3(QSV_BLOCK), 0, psi->stream, psi->data, lambda->data,
                           static_cast<const double *>(d->data), static_cast<const double *>(psi->dev_matrix), e, partials);
    });
    snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_ens_diag_phase_adjoint<%s>", nt ? "true" : "false");
    rc = check_launch();
    if (rc) return rc;
    // the copy waits for the kernel on psi's stream: both registers are finished when the call returns
    return fetch_pair_sums(psi, e, partials, slots, values);
}

}  // extern "C"

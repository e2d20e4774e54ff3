// Parameter ensembles (gfx950, wave64): every member of an ensemble (qsv_ensemble_layout.h) takes its own angles through a
// Pauli-rotation list, its own gamma through a diagonal cost phase, and reads back its own moments of the diagonal
// (DESIGN.md section 27).  Per-member dense matrices need no kernel of their own: qsv_ensemble_apply_matrices in
// qsv_ensemble.hip fills the matrix slots of k_ens_channel_apply.
//   k_ens_pauli_rotate_group  k_pauli_rotate_group on member-local items, cos / sin from a device table [members][n_terms][2];
//   k_ens_diag_phase          k_diag_phase with the member's gamma and the diagonal indexed by the member-local index;
//   k_ens_diag_expect         k_diag_expect's accumulation per member and part, ended by member_store_sums and k_ens_sum_parts.
// The per-item arithmetic is the single-register kernels' own (qsv_pauli_rotate_item.h, qsv_diagonal_device.h): a member
// rounds exactly as a register of its own would.  Launch shapes: qsv_sweep_layout.h.

#include "qsv_device.h"
#include "qsv_diagonal_device.h"
#include "qsv_ensemble_device.h"
#include "qsv_pauli_rotate_item.h"
#include "qsv_sweep_layout.h"

#include <cmath>
#include <vector>

using namespace qsv_ensemble_layout;
using namespace qsv_sweep_layout;
using qsv_readout_layout::pauli_rotate_args;
using qsv_readout_layout::PauliRotate;
using qsv_readout_layout::PauliRotateArgs;

namespace {

// k_pauli_rotate_group's item loop on the items of one member: work item w of member m owns amplitude w of the member (DIAG)
// or the pair {i, i ^ xmask}, i = insert_zero(w, pivot), inside a + (m << n); pivot <= n - 1, so the partner stays in the
// member.  The member's cos / sin of the pass's s.count terms replace g.cs / g.sn (never read here: the slots beyond the
// count get the padding of pauli_rotate_args, theta = 0, spelled out); they are fetched once per unit, before the item
// loop -- all T slots without a branch: the table ends in TABLE_PAD doubles so that the slots beyond the count of the last
// member's last pass are inside the allocation.  WAVE: a wave lies in one member (64 items or more per member) and the
// member index is made provably wave-uniform, so the fetch is a scalar load; otherwise members share a wave and every lane
// fetches its own.  No LDS, no barrier, in place.
template <int T, bool DIAG, bool NT, bool WAVE>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_pauli_rotate_group(amp_t *__restrict__ a, const PauliRotateArgs g, const EnsArgs e, const SweepArgs s,
                                                                      const double *__restrict__ table) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        if (!t.live) continue;     // no barrier in this kernel
        const uint64_t member = WAVE ? wave_uniform(t.member) : t.member;
        const double *row = table + member * s.row_doubles + s.first;
        PauliRotateArgs h = g;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const double c = row[2 * k], sn = row[2 * k + 1];
            h.cs[k] = k < s.count ? c : 1.0;
            h.sn[k] = k < s.count ? sn : 0.0;
        }
        amp_t *am = a + (member << e.n);
        for (uint64_t w = t.first; w < t.items; w += t.stride) {
            const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
            amp_t x = ld<NT>(am + i), y = amp_t{0.0, 0.0};
            if constexpr (!DIAG) y = ld<NT>(am + (i ^ g.xmask));
            pauli_rotate_item<T, DIAG>(h, i, x, y);
            st<NT>(am + i, x);
            if constexpr (!DIAG) st<NT>(am + (i ^ g.xmask), y);
        }
    }
}

// psi_m[i] *= exp(-i gammas[m] d[i]): a flat loop over the register.  The diagonal is read once per member and the gammas
// once per amplitude, both through the caches; the register streams.
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_diag_phase(amp_t *__restrict__ psi, const double *__restrict__ d, const double *__restrict__ gammas,
                                                              uint64_t amps, int n) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK, mask = (1ull << n) - 1ull;
    for (uint64_t idx = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; idx < amps; idx += stride) {
        const amp_t v = ld<NT>(psi + idx);
        const double x = d[idx & mask];
        st<NT>(psi + idx, cmul(phase_of(gammas[idx >> n], x), v));
    }
}

// partials[member][part][4] = the part's share of { sum p, sum p d, sum p d^2, sum_{d <= threshold} p } over the member,
// p = |psi_m[i]|^2: k_diag_expect's accumulation on the units of a read pass.  THR = false: slot 3 is 0.  Read-only.
template <bool THR>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_diag_expect(const amp_t *__restrict__ a, const double *__restrict__ d, const EnsArgs e, double threshold,
                                                               double *__restrict__ partials) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        double v[SWEEP_EXPECT_SLOTS] = {0.0, 0.0, 0.0, 0.0};
        if (t.live) {
            const amp_t *am = a + (t.member << e.n);
            for (uint64_t w = t.first; w < t.items; w += t.stride) {
                const amp_t y = am[w];
                const double x = d[w];
                const double p = fma(y.x, y.x, y.y * y.y);
                const double px = p * x;
                v[0] += p;
                v[1] += px;
                v[2] = fma(px, x, v[2]);
                if constexpr (THR) v[3] += x <= threshold ? p : 0.0;
            }
        }
        member_store_sums<SWEEP_EXPECT_SLOTS>(v, e, t, partials);
    }
}

bool all_finite(const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// A register and a diagonal of member size that can meet in one pass.
int check_member_diag(const qsv_state *st, int member_qubits, const qsv_diag *d) {
    if (st->device != d->device) return qsv_fail(QSV_EINVAL, "register and diagonal on different devices");
    if (d->n != member_qubits || d->size != (1ull << member_qubits))
        return qsv_fail(QSV_EINVAL, "the diagonal must have the size of a member (" + std::to_string(member_qubits) + " qubits), not " + std::to_string(d->n));
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_ensemble_apply_pauli_rotations(qsv_state *st, int member_qubits, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                                       const double *thetas, uint64_t *passes) {
    if (!st) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_terms < 0) return qsv_fail(QSV_EINVAL, "negative number of Pauli terms");
    if (n_terms > 0 && (!term_offsets || !thetas)) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    // the whole list is checked and turned into masks of member bits before the queue is flushed or anything is launched
    const int n = member_qubits;
    std::vector<qsv_pauli_plan::Term> terms;
    rc = parse_member_terms(n, n_terms, term_offsets, qubits, paulis, &terms);
    if (rc) return rc;
    const uint64_t members = st->amps >> n;
    if (n_terms > 0 && !all_finite(thetas, static_cast<size_t>(members) * n_terms)) return qsv_fail(QSV_EINVAL, "every angle must be finite");
    if (passes) *passes = 0;
    if (n_terms == 0) return QSV_OK;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    // cos / sin with the expressions of qsv_apply_pauli_rotations, one row per member
    const size_t doubles = table_doubles(members, n_terms);
    std::vector<double> host(doubles, 0.0);
    for (size_t i = 0; i < static_cast<size_t>(members) * n_terms; ++i) {
        host[2 * i] = std::cos(0.5 * thetas[i]);
        host[2 * i + 1] = std::sin(0.5 * thetas[i]);
    }
    rc = qsvk_ensure_matrix(st, sizeof(double) * doubles);
    if (rc) return rc;
    // pageable memory: the copy has left `host` when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(st->dev_matrix, host.data(), sizeof(double) * doubles, hipMemcpyHostToDevice, st->stream));
    const std::vector<qsv_pauli_rotation_plan::Pass> plan = qsv_pauli_rotation_plan::plan(terms);
    const std::vector<double> ones(static_cast<size_t>(n_terms), 1.0), zeros(static_cast<size_t>(n_terms), 0.0);
    for (const qsv_pauli_rotation_plan::Pass &p : plan) {
        // the pass on a register of one member: items, masks, what each term is; theta = 0 in every slot, the table has the rest
        const PauliRotate r = pauli_rotate_args(p, 1ull << n, ones.data(), zeros.data());
        if (!r.ok) return qsv_fail(QSV_EINVAL, "bad Pauli rotation pass");
        const bool diag = p.pivot < 0;
        const bool nt = rotate_nontemporal(st->nontemporal != 0, diag, p.pivot);
        const EnsArgs e = rotate_args(n, members, diag, st->grid_cap);
        const bool wave = wave_in_one_member(e);
        const SweepArgs s = sweep_args(n_terms, p.index.front(), static_cast<int>(p.index.size()));
        const dim3 gd(ens_grid(e, st->grid_cap)), bd(QSV_BLOCK);
        with_pow2<1, 8>(r.width, [&](auto W) { with_bool(diag, [&](auto DIAG) { with_bool(nt, [&](auto NT) { with_bool(wave, [&](auto WAVE) {
            hipLaunchKernelGGL((k_ens_pauli_rotate_group<W.value, DIAG.value, NT.value, WAVE.value>), gd, bd, 0, st->stream, st->data, r.g, e, s,
                               static_cast<const double *>(st->dev_matrix));
        }); }); }); });
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_pauli_rotate_group<%d, %s, %s, %s>", r.width, diag ? "true" : "false",
                 nt ? "true" : "false", wave ? "true" : "false");
        rc = check_launch();
        if (rc) return rc;
    }
    if (passes) *passes = plan.size();
    return QSV_OK;
}

int qsv_ensemble_apply_diag_phase(qsv_state *st, int member_qubits, qsv_diag *d, const double *gammas) {
    if (!st || !d || !gammas) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    rc = check_member_diag(st, member_qubits, d);
    if (rc) return rc;
    const uint64_t members = st->amps >> member_qubits;
    if (!all_finite(gammas, members)) return qsv_fail(QSV_EINVAL, "every gamma must be finite");
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = wait_for_diag(d, st->stream);
    if (rc) return rc;
    rc = qsvk_ensure_matrix(st, sizeof(double) * members);
    if (rc) return rc;
    // pageable memory: the copy has left the caller's array when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(st->dev_matrix, gammas, sizeof(double) * members, hipMemcpyHostToDevice, st->stream));
    const bool nt = st->nontemporal != 0;
    const dim3 gd(qsv_diagonal_layout::stream_grid(st->amps, st->grid_cap)), bd(QSV_BLOCK);
    with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_ens_diag_phase<NT.value>), gd, bd, 0, st->stream, st->data, static_cast<const double *>(d->data),
                           static_cast<const double *>(st->dev_matrix), st->amps, member_qubits);
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_diag_phase<%s>", nt ? "true" : "false");
    return check_launch();
}

int qsv_ensemble_expect_diag(qsv_state *st, int member_qubits, qsv_diag *d, const double *threshold, double *out) {
    if (!st || !d || !out) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    rc = check_member_diag(st, member_qubits, d);
    if (rc) return rc;
    if (threshold && !std::isfinite(*threshold)) return qsv_fail(QSV_EINVAL, "the threshold must be finite");
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = wait_for_diag(d, st->stream);
    if (rc) return rc;
    const uint64_t members = st->amps >> member_qubits;
    const EnsArgs e = expect_args(member_qubits, members, st->grid_cap);
    rc = qsvk_ensure_matrix(st, sizeof(double) * expect_doubles(e));
    if (rc) return rc;
    double *values = st->dev_matrix, *partials = st->dev_matrix + expect_values(members);
    const double thr = threshold ? *threshold : 0.0;
    with_bool(threshold != nullptr, [&](auto THR) {
        hipLaunchKernelGGL((k_ens_diag_expect<THR.value>), dim3(ens_grid(e, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           static_cast<const amp_t *>(st->data), static_cast<const double *>(d->data), e, thr, partials);
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_diag_expect<%s>", threshold ? "true" : "false");
    rc = check_launch();
    if (rc) return rc;
    rc = qsvk_ens_sum_parts(st, partials, members, 1 << e.part_bits, SWEEP_EXPECT_SLOTS, values);
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(out, values, sizeof(double) * expect_values(members), hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

}  // extern "C"

// Trajectory ensembles (gfx950, wave64): 2^b independent n-qubit kets side by side in one (n + b)-qubit register, member m at
// the amplitudes [m 2^n, (m + 1) 2^n), and the member-wise forms of the steps that do not batch by themselves (DESIGN.md
// section 23).  A general channel call is two passes over the register and no host synchronisation:
//   k_ens_channel_rdm     reads the register once and leaves, per member and part, that part's share of the member's reduced
//                         density matrix of the target qubits (real numbers, rdm_pair_slot order);
//   k_ens_channel_select  16 threads per member: the member's parts added in index order, then k_channel_select's steps one
//                         for one -- weights, the choice against the member's own draw, K_j sqrt(total / w_j) into the
//                         member's matrix slot, (j, w_j / total) into the member's column of the device log;
//   k_ens_channel_apply   one in-place pass, every group of 2^k amplitudes multiplied by the matrix of its own member.
// A measurement is the same two passes around k_ens_measure_select, which has the two eigenvectors in
// its kernel arguments, takes the member's outcome by the same rule and writes it to one of the member's 64 classical bits;
// k_ens_apply_conditional is k_ens_channel_apply with one matrix for all members and a predicate on those bits: members
// that do not take the gate are neither read nor written.
// qsv_ensemble_apply_matrices is k_ens_channel_apply with the matrix slots filled by the caller.
// k_ens_expect_pauli_group / k_ens_sum_parts give <psi_m|P_t|psi_m> per member for the passes of qsv_pauli_plan.h.
// The per-item bodies are those of k_channel_rdm, k_channel_apply and k_expect_pauli_group on a register of 2^n amplitudes;
// what is new is the member dimension and where the sums stop.  Launch shapes: qsv_ensemble_layout.h.

#include "qsv_device.h"
#include "qsv_ensemble_device.h"
#include "qsv_ensemble_control_layout.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace qsv_channel_layout;
using namespace qsv_ensemble_layout;
using qsv_ensemble_control_layout::ConditionalArgs;
using qsv_ensemble_control_layout::cond_grid;
using qsv_ensemble_control_layout::MeasureArgs;
using qsv_readout_layout::PauliPass;
using qsv_readout_layout::PauliPassArgs;
using qsv_readout_layout::pauli_pass_args;

static_assert(CH_BLOCK == QSV_BLOCK && CH_LANE_BITS == QSV_LANE_BITS, "qsv_channel_layout.h mirrors qsv_internal.h");

namespace {

// A register's ensemble workspace (device), its pinned ring of draws and its branch log.  Every step of the log is chosen on
// the device: the first `host_steps` steps are already in host memory, the next `used` sit in the device slots 0 .. used-1.
struct EnsembleWork {
    int device = 0;
    int n = -1;                       // member qubits the workspace was sized for
    EnsWorkspace ws;
    double *dev = nullptr;            // ws.doubles doubles
    double *ring = nullptr;           // pinned host: [ws.slots][members][2], the draws of the step that will fill that log slot
    int used = 0;
    std::vector<int32_t> branches;    // [host steps][members]
    std::vector<double> probs;
    uint64_t *bits = nullptr;         // device: one word of classical bits per member, an allocation of its own
    int bits_n = -1;                  // member qubits and members the words were made for
    uint64_t bits_members = 0;
};

void free_ensemble_work(void *p) {
    EnsembleWork *w = static_cast<EnsembleWork *>(p);
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->dev) (void)hipFree(w->dev);
    if (w->ring) (void)hipHostFree(w->ring);
    if (w->bits) (void)hipFree(w->bits);
    delete w;
}

EnsembleWork *work_of(qsv_state *st) {
    if (!st->ensemble_work) {
        EnsembleWork *w = new EnsembleWork;
        w->device = st->device;
        st->ensemble_work = w;
        st->ensemble_work_free = free_ensemble_work;
    }
    return static_cast<EnsembleWork *>(st->ensemble_work);
}

uint64_t pending_steps(const EnsembleWork *w) { return w->ws.members ? w->branches.size() / w->ws.members + w->used : 0; }

// Device log -> host entries.  One copy and one synchronisation; the only time qsv_ensemble_apply_channel may wait.
int drain(qsv_state *st, EnsembleWork *w) {
    if (w->used == 0) return QSV_OK;
    const size_t count = static_cast<size_t>(w->used) * w->ws.members;
    std::vector<double> host(2 * count);
    QSV_HIP(hipMemcpyAsync(host.data(), w->dev + w->ws.log, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    for (size_t e = 0; e < count; ++e) {
        w->branches.push_back(static_cast<int32_t>(host[2 * e]));
        w->probs.push_back(host[2 * e + 1]);
    }
    w->used = 0;
    return QSV_OK;
}

// Sized at the first call; re-made when the member size changes (only with an empty log: its rows have `members` columns).
int ensure_workspace(qsv_state *st, EnsembleWork *w, int n, uint64_t members) {
    if (w->dev && w->n == n && w->ws.members == members) return QSV_OK;
    QSV_HIP(hipStreamSynchronize(st->stream));
    if (w->dev) (void)hipFree(w->dev);
    if (w->ring) (void)hipHostFree(w->ring);
    w->dev = nullptr;
    w->ring = nullptr;
    w->n = -1;
    const EnsWorkspace ws = ens_workspace(n, members);
    if (hipMalloc(reinterpret_cast<void **>(&w->dev), sizeof(double) * ws.doubles) != hipSuccess) {
        w->dev = nullptr;
        return qsv_fail(QSV_ENOMEM, "device allocation of the ensemble workspace failed");
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&w->ring), sizeof(double) * 2 * members * ws.slots, hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(w->dev);
        w->dev = nullptr;
        w->ring = nullptr;
        return qsv_fail(QSV_ENOMEM, "pinned allocation of the ensemble draws failed");
    }
    w->ws = ws;
    w->n = n;
    w->used = 0;
    return QSV_OK;
}

// The classical bits: made and zeroed at the first call that needs them, re-made and zeroed when the member size changes.
int ensure_bits(qsv_state *st, EnsembleWork *w, int n, uint64_t members) {
    if (w->bits && w->bits_n == n && w->bits_members == members) return QSV_OK;
    if (w->bits) {
        QSV_HIP(hipStreamSynchronize(st->stream));
        (void)hipFree(w->bits);
        w->bits = nullptr;
    }
    if (hipMalloc(reinterpret_cast<void **>(&w->bits), qsv_ensemble_control_layout::bits_bytes(members)) != hipSuccess) {
        w->bits = nullptr;
        return qsv_fail(QSV_ENOMEM, "device allocation of the ensemble's classical bits failed");
    }
    w->bits_n = n;
    w->bits_members = members;
    QSV_HIP(hipMemsetAsync(w->bits, 0, qsv_ensemble_control_layout::bits_bytes(members), st->stream));
    return QSV_OK;
}

// the member size may change only while the log is empty: its rows have `members` columns
int check_member_size(const EnsembleWork *w, int n, uint64_t members) {
    if (w->dev && (w->n != n || w->ws.members != members) && pending_steps(w) > 0)
        return qsv_fail(QSV_ESTATE, "read the ensemble log before changing the member size");
    return QSV_OK;
}

// ---- device -----------------------------------------------------------------------------------------------------------------

// x conj(y)
__device__ __forceinline__ amp_t mul_conj(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.y, y.x, -(x.x * y.y))};
}
template <int KL>
__device__ __forceinline__ int glo_of(const ChannelArgs &g, int l) {
    int v = 0;
    if constexpr (KL >= 1) v |= (l & 1) ? g.glo[1] : 0;
    if constexpr (KL >= 2) v |= (l & 2) ? g.glo[2] : 0;
    return v;
}
template <int KL>
__device__ __forceinline__ int own_combination(const ChannelArgs &g) {
    const int lane = threadIdx.x & 63;
    int l = 0;
    if constexpr (KL >= 1) l |= (lane >> g.lbit[0]) & 1;
    if constexpr (KL >= 2) l |= ((lane >> g.lbit[1]) & 1) << 1;
    return l;
}

// Mine / mine (who works on what in a unit) and member_store_sums: qsv_ensemble_device.h, shared with qsv_sweep.hip.

// k_channel_rdm's item body on member-local indices.  Read-only.
template <int K, int KL, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_channel_rdm(const amp_t *__restrict__ a, const ChannelArgs g, const EnsArgs e,
                                                               double *__restrict__ partials) {
    constexpr int KH = K - KL, NH = 1 << KH, NL = 1 << KL, D = 1 << K, R = D * D;
    const int l_own = own_combination<KL>(g);
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        amp_t acc[NH][NH][NL];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int dl = 0; dl < NL; ++dl) acc[h][j][dl] = amp_t{0.0, 0.0};
        if (t.live) {
            // KL > 0: the items of a member are a multiple of 64 and `live` is the same for a whole wave: a wave is in the
            // loop as a whole
            const amp_t *am = a + (t.member << e.n);
            for (uint64_t w = t.first; w < t.items; w += t.stride) {
                const uint64_t base = deposit(w, g);
                amp_t x[NH];
#pragma unroll
                for (int h = 0; h < NH; ++h) x[h] = ld<NT>(am + base + g.hoff[h]);
#pragma unroll
                for (int j = 0; j < NH; ++j)
#pragma unroll
                    for (int dl = 0; dl < NL; ++dl) {
                        const amp_t y = dl == 0 ? x[j] : shfl_xor_amp(x[j], g.lxor[dl]);
#pragma unroll
                        for (int h = 0; h < NH; ++h) {
                            if (KL == 0 && h > j) continue;
                            const amp_t p = mul_conj(x[h], y);
                            acc[h][j][dl].x += p.x;
                            acc[h][j][dl].y += p.y;
                        }
                    }
            }
        }
        double v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int dl = 0; dl < NL; ++dl) {
                    if (KL == 0 && h > j) continue;
                    int r = g.ghi[h] | glo_of<KL>(g, l_own), c = g.ghi[j] | glo_of<KL>(g, l_own ^ dl);
                    const double re = acc[h][j][dl].x;
                    double im = acc[h][j][dl].y;
                    if (KL == 0 && r > c) {
                        const int s = r;
                        r = c;
                        c = s;
                        im = -im;
                    }
                    int slot = D;      // rdm_pair_slot, walked in its own order
#pragma unroll
                    for (int rr = 0; rr < D; ++rr) {
                        v[rr] += (r == rr && c == rr) ? re : 0.0;
#pragma unroll
                        for (int cc = rr + 1; cc < D; ++cc) {
                            const bool hit = r == rr && c == cc;
                            v[slot] += hit ? re : 0.0;
                            v[slot + 1] += hit ? im : 0.0;
                            slot += 2;
                        }
                    }
                }
        member_store_sums<R>(v, e, t, partials);
    }
}

// 16 threads per member, 16 members per workgroup.  partials: [members][P][R] (unused for a mixed-unitary channel, whose
// weights are the stored p_j = E_j[0][0]); chan: K_0 .. K_{n-1} then E_0 .. E_{n-1}; draws: [members][2] = u, forced branch
// (-1: draw); matrix: [members][32]; log: [members][2] of this step.  The steps of k_channel_select, one member per group.
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_channel_select(const double *__restrict__ partials, int parts, const double *__restrict__ chan,
                                                                  int n_kraus, int D, int mixed, const double *__restrict__ draws, uint64_t members,
                                                                  double *__restrict__ matrix, double *__restrict__ log) {
    constexpr int GROUPS = QSV_BLOCK / ENS_SELECT_LANES;
    __shared__ double rho[GROUPS][16];
    __shared__ double wt[GROUPS][CH_MAX_KRAUS];
    __shared__ int chosen[GROUPS];
    __shared__ double scale[GROUPS];
    const int s = threadIdx.x / ENS_SELECT_LANES, t = threadIdx.x % ENS_SELECT_LANES, DD = D * D;
    for (uint64_t first = static_cast<uint64_t>(blockIdx.x) * GROUPS; first < members; first += static_cast<uint64_t>(gridDim.x) * GROUPS) {
        const uint64_t m = first + s;
        const bool live = m < members;
        if (live && !mixed && t < DD) {
            const double *p = partials + m * parts * DD + t;
            double sum = 0.0;
            for (int q = 0; q < parts; ++q) sum += p[static_cast<size_t>(q) * DD];      // index order
            rho[s][t] = sum;
        }
        __syncthreads();
        if (live && t < n_kraus) {
            const double *E = chan + 2 * static_cast<size_t>(DD) * (n_kraus + t);
            if (mixed) {
                wt[s][t] = E[0];
            } else {
                double d = 0.0;
                for (int r = 0; r < D; ++r) d += E[2 * (r * D + r)] * rho[s][r];
                int slot = D;
                double off = 0.0;
                for (int r = 0; r < D; ++r)
                    for (int c = r + 1; c < D; ++c) {
                        off += E[2 * (r * D + c)] * rho[s][slot] + E[2 * (r * D + c) + 1] * rho[s][slot + 1];
                        slot += 2;
                    }
                wt[s][t] = d + 2.0 * off;
            }
        }
        __syncthreads();
        if (live && t == 0) {
            double total = 0.0;
            for (int j = 0; j < n_kraus; ++j) total += wt[s][j];
            const double u = draws[2 * m];
            int pick = static_cast<int>(draws[2 * m + 1]);
            if (pick < 0) {
                const double target = u * total;
                double run = 0.0;
                int last = -1;
                for (int j = 0; j < n_kraus && pick < 0; ++j) {
                    run += wt[s][j];
                    if (wt[s][j] > 0.0) last = j;
                    if (run > target && wt[s][j] > 0.0) pick = j;
                }
                if (pick < 0) pick = last < 0 ? 0 : last;
            }
            const double wj = wt[s][pick];
            const bool alive = wj > 0.0 && total > 0.0;
            chosen[s] = pick;
            scale[s] = alive ? sqrt(total / wj) : 0.0;
            log[2 * m] = static_cast<double>(pick);
            log[2 * m + 1] = alive ? wj / total : 0.0;
        }
        __syncthreads();
        if (live && t < DD) {
            const double *Kj = chan + 2 * static_cast<size_t>(DD) * chosen[s];
            const double sc = scale[s];
            // a scale of 0 writes zeros whatever K_j holds (0 * inf would not)
            matrix[32 * m + 2 * t] = sc != 0.0 ? Kj[2 * t] * sc : 0.0;
            matrix[32 * m + 2 * t + 1] = sc != 0.0 ? Kj[2 * t + 1] * sc : 0.0;
        }
        __syncthreads();     // the next round writes the shared arrays again
    }
}

// k_channel_apply's item body on member-local indices, with the matrix of the thread's own member.  Where a unit lies in one
// member (256 items or more) the member index is the same for the whole workgroup and the entries are fetched once per unit,
// before the item loop; where members share a unit the index differs between the threads of a wave and each fetches its own.
template <int K, int KL, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_channel_apply(amp_t *__restrict__ a, const ChannelArgs g, const EnsArgs e,
                                                                 const double *__restrict__ matrix) {
    constexpr int KH = K - KL, NH = 1 << KH, NL = 1 << KL, D = 1 << K;
    const int l_own = own_combination<KL>(g);
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        if (!t.live) continue;     // whole waves (KL > 0), and no barrier in this kernel
        const double *m = matrix + 32 * t.member;
        cplx mm[NH][NH][NL];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int dl = 0; dl < NL; ++dl) {
                    const int r = g.ghi[h] | glo_of<KL>(g, l_own), c = g.ghi[j] | glo_of<KL>(g, l_own ^ dl);
                    mm[h][j][dl] = cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]};
                }
        amp_t *am = a + (t.member << e.n);
        for (uint64_t w = t.first; w < t.items; w += t.stride) {
            const uint64_t base = deposit(w, g);
            amp_t x[NH], out[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                x[h] = ld<NT>(am + base + g.hoff[h]);
                out[h] = amp_t{0.0, 0.0};
            }
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int dl = 0; dl < NL; ++dl) {
                    const amp_t y = dl == 0 ? x[j] : shfl_xor_amp(x[j], g.lxor[dl]);
#pragma unroll
                    for (int h = 0; h < NH; ++h) out[h] = cfma(mm[h][j][dl], y, out[h]);
                }
#pragma unroll
            for (int h = 0; h < NH; ++h) st<NT>(am + base + g.hoff[h], out[h]);
        }
    }
}

// One thread per member.  The steps of k_ens_channel_select for the two rank-1 operators K_s = v_s e_s^T of a measurement,
// E_s = K_s^dagger K_s = conj(e_s) e_s^T: the member's parts added in index order, w_s = tr(E_s rho), the choice against
// the member's own draw, K_s sqrt(total / w_s) into the member's matrix slot, (s, w_s / total) into the member's column of
// the log -- and the outcome into bit c.bit of the member's word (a plain store: nobody else writes that word).
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_measure_select(const double *__restrict__ partials, int parts, const MeasureArgs c,
                                                                  const double *__restrict__ draws, uint64_t members, double *__restrict__ matrix,
                                                                  double *__restrict__ log, uint64_t *__restrict__ bits) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t m = static_cast<uint64_t>(blockIdx.x) * QSV_BLOCK + threadIdx.x; m < members; m += stride) {
        double rho[4] = {0.0, 0.0, 0.0, 0.0};     // rho00, rho11, Re rho01, Im rho01
        const double *p = partials + m * parts * 4;
        for (int q = 0; q < parts; ++q)            // index order
#pragma unroll
            for (int r = 0; r < 4; ++r) rho[r] += p[static_cast<size_t>(q) * 4 + r];
        double wt[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double ar = c.eig[s][0], ai = c.eig[s][1], br = c.eig[s][2], bi = c.eig[s][3];
            const double d = (ar * ar + ai * ai) * rho[0] + (br * br + bi * bi) * rho[1];
            const double off = (ar * br + ai * bi) * rho[2] + (ar * bi - ai * br) * rho[3];     // E01 = conj(e[0]) e[1]
            wt[s] = d + 2.0 * off;
        }
        const double total = wt[0] + wt[1];
        const double u = draws[2 * m];
        int pick = static_cast<int>(draws[2 * m + 1]);
        if (pick < 0) {
            const double target = u * total;
            double run = 0.0;
            int last = -1;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                run += wt[j];
                if (wt[j] > 0.0) last = j;
                if (pick < 0 && run > target && wt[j] > 0.0) pick = j;
            }
            if (pick < 0) pick = last < 0 ? 0 : last;
        }
        const double wj = pick ? wt[1] : wt[0];
        const bool alive = wj > 0.0 && total > 0.0;
        const double sc = alive ? sqrt(total / wj) : 0.0;
        log[2 * m] = static_cast<double>(pick);
        log[2 * m + 1] = alive ? wj / total : 0.0;
        // K[r][c] = v[r] e[c] sc, v = conj(e) (keep) or |0> (reset); a scale of 0 writes zeros whatever e holds
        const double er[2] = {pick ? c.eig[1][0] : c.eig[0][0], pick ? c.eig[1][2] : c.eig[0][2]};
        const double ei[2] = {pick ? c.eig[1][1] : c.eig[0][1], pick ? c.eig[1][3] : c.eig[0][3]};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double vr = c.after ? (r == 0 ? 1.0 : 0.0) : er[r], vi = c.after ? 0.0 : -ei[r];
#pragma unroll
            for (int col = 0; col < 2; ++col) {
                matrix[32 * m + 2 * (r * 2 + col)] = sc != 0.0 ? (vr * er[col] - vi * ei[col]) * sc : 0.0;
                matrix[32 * m + 2 * (r * 2 + col) + 1] = sc != 0.0 ? (vr * ei[col] + vi * er[col]) * sc : 0.0;
            }
        }
        if (c.bit >= 0) {
            const uint64_t mask = 1ull << c.bit, word = bits[m];
            bits[m] = pick ? word | mask : word & ~mask;
        }
    }
}

// k_ens_channel_apply's item body and index arithmetic with ONE matrix, in the kernel arguments and fetched once, for the
// members whose classical bits satisfy (word & all_of) == all_of && (word & none_of) == 0.  Where a unit lies in one member
// (256 items or more) the member index comes from the unit, the word is loaded once per unit -- a chunk of units per load -- and the
// whole workgroup skips the unit; where members share a unit every thread tests the word of its own member.  With KL > 0 a wave lies in one
// member (n >= 6), so every shfl_xor partner of a lane has the lane's predicate and a wave is in the item loop as a whole
// (cond_partner_member of qsv_ensemble_control_layout.h).  No barrier.  A member that does not take the gate is neither
// read nor written.
template <int K, int KL, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_apply_conditional(amp_t *__restrict__ a, const ChannelArgs g, const EnsArgs e, const ConditionalArgs c,
                                                                     const uint64_t *__restrict__ bits) {
    constexpr int KH = K - KL, NH = 1 << KH, NL = 1 << KL, D = 1 << K;
    const int l_own = own_combination<KL>(g);
    cplx mm[NH][NH][NL];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int dl = 0; dl < NL; ++dl) {
                const int r = g.ghi[h] | glo_of<KL>(g, l_own), col = g.ghi[j] | glo_of<KL>(g, l_own ^ dl);
                mm[h][j][dl] = cplx{c.m[2 * (r * D + col)], c.m[2 * (r * D + col) + 1]};
            }
    // the items of unit `unit` that are this thread's
    auto work = [&](const Mine &t) {
        amp_t *am = a + (t.member << e.n);
        for (uint64_t w = t.first; w < t.items; w += t.stride) {
            const uint64_t base = deposit(w, g);
            amp_t x[NH], out[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                x[h] = ld<NT>(am + base + g.hoff[h]);
                out[h] = amp_t{0.0, 0.0};
            }
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int dl = 0; dl < NL; ++dl) {
                    const amp_t y = dl == 0 ? x[j] : shfl_xor_amp(x[j], g.lxor[dl]);
#pragma unroll
                    for (int h = 0; h < NH; ++h) out[h] = cfma(mm[h][j][dl], y, out[h]);
                }
#pragma unroll
            for (int h = 0; h < NH; ++h) st<NT>(am + base + g.hoff[h], out[h]);
        }
    };
    if (e.item_bits >= ENS_BLOCK_BITS) {
        // A unit lies in one member.  A workgroup takes chunks of 2^chunk_bits consecutive units: lane l of every wave fetches
        // the word of unit (chunk << chunk_bits) + l (cond_batch_unit), the ballot is the same wave-uniform mask in all four
        // waves, and the workgroup works through the units whose bit is set: a unit that is skipped costs nothing but its
        // share of this load.
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t chunks = (e.units + (1ull << c.chunk_bits) - 1ull) >> c.chunk_bits;
        for (uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
            const uint64_t first = chunk << c.chunk_bits, candidate = first + lane;
            bool take = false;
            if (lane < (1u << c.chunk_bits) && candidate < e.units) {
                const uint64_t word = bits[(candidate >> e.part_bits) << e.share_bits];
                take = (word & c.all_of) == c.all_of && (word & c.none_of) == 0;
            }
            unsigned long long todo = __ballot(take);
            while (todo) {
                const int l = __ffsll(todo) - 1;
                todo &= todo - 1;
                work(mine(e, first + static_cast<uint64_t>(l)));     // live: with 256 items or more per member every unit is
            }
        }
        return;
    }
    // Members share a unit: every thread tests the word of its own member (whole waves where KL > 0)
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        if (!t.live) continue;
        const uint64_t word = bits[t.member];
        if ((word & c.all_of) != c.all_of || (word & c.none_of) != 0) continue;
        work(t);
    }
}

// k_expect_pauli_group's item body on member-local indices (g.items is not used: the items of a member are e.item_bits).
constexpr int ENS_PAULI_ITEMS = 4;
template <int T, bool DIAG>
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_expect_pauli_group(const amp_t *__restrict__ a, const PauliPassArgs g, const EnsArgs e,
                                                                     double *__restrict__ partials) {
    for (uint64_t unit = blockIdx.x; unit < e.units; unit += gridDim.x) {
        const Mine t = mine(e, unit);
        double acc[T];
#pragma unroll
        for (int k = 0; k < T; ++k) acc[k] = 0.0;
        auto add = [&](uint64_t i, double re, double im) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const double v = (!DIAG && ((g.odd >> k) & 1u)) ? im : re;
                acc[k] += (__popcll(i & g.zmask[k]) & 1) ? -v : v;
            }
        };
        if (t.live) {
            const amp_t *am = a + (t.member << e.n);
            uint64_t w = t.first;
            // ENS_PAULI_ITEMS independent items are loaded before any is used, as in k_expect_pauli_group; they are added in
            // item order, so the sums are those of the plain loop below
            for (; w + (ENS_PAULI_ITEMS - 1) * t.stride < t.items; w += ENS_PAULI_ITEMS * t.stride) {
                uint64_t i[ENS_PAULI_ITEMS];
                amp_t x[ENS_PAULI_ITEMS], y[ENS_PAULI_ITEMS];
#pragma unroll
                for (int u = 0; u < ENS_PAULI_ITEMS; ++u) {
                    i[u] = DIAG ? w + u * t.stride : insert_zero(w + u * t.stride, g.pivot);
                    y[u] = am[i[u]];
                    if constexpr (!DIAG) x[u] = am[i[u] ^ g.xmask];
                }
#pragma unroll
                for (int u = 0; u < ENS_PAULI_ITEMS; ++u) {
                    if constexpr (DIAG) add(i[u], y[u].x * y[u].x + y[u].y * y[u].y, 0.0);
                    else add(i[u], x[u].x * y[u].x + x[u].y * y[u].y, x[u].x * y[u].y - x[u].y * y[u].x);   // conj(x) * y
                }
            }
            for (; w < t.items; w += t.stride) {
                const uint64_t i = DIAG ? w : insert_zero(w, g.pivot);
                const amp_t y = am[i];
                if constexpr (DIAG) {
                    add(i, y.x * y.x + y.y * y.y, 0.0);
                } else {
                    const amp_t x = am[i ^ g.xmask];
                    add(i, x.x * y.x + x.y * y.y, x.x * y.y - x.y * y.x);
                }
            }
        }
        member_store_sums<T>(acc, e, t, partials);
    }
}

// out[m * R + r] = sum over the parts of member m of partials[(m * P + p) * R + r], in index order
__global__ __launch_bounds__(QSV_BLOCK) void k_ens_sum_parts(const double *__restrict__ partials, uint64_t members, int parts, int R,
                                                             double *__restrict__ out) {
    const uint64_t count = members * R, stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < count; i += stride) {
        const uint64_t m = i / R;
        const int r = static_cast<int>(i % R);
        const double *p = partials + m * parts * R + r;
        double sum = 0.0;
        for (int q = 0; q < parts; ++q) sum += p[static_cast<size_t>(q) * R];
        out[i] = sum;
    }
}

template <class F>
void with_shape(int k, int kl, bool nt, F &&f) {
    with_bool(nt, [&](auto NT) {
        if (k == 1 && kl == 0) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, NT);
        else if (k == 1) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, NT);
        else if (kl == 0) f(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, NT);
        else if (kl == 1) f(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, NT);
        else f(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, NT);
    });
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

// check_ensemble / check_member_qubits (what every ensemble call refuses): qsv_ensemble_device.h.

// values[pass offset + m * width + t] for every pass, summed per member on the device; one copy, one synchronisation
int expect_passes(qsv_state *st, int n, const std::vector<qsv_pauli_plan::Pass> &passes, std::vector<double> *host, std::vector<size_t> *offsets,
                  std::vector<int> *widths) {
    const uint64_t members = st->amps >> n;
    size_t doubles = 0, most_partials = 0;
    struct Launch { PauliPass pass; EnsArgs e; };
    std::vector<Launch> launches;
    for (const qsv_pauli_plan::Pass &p : passes) {
        const PauliPass pass = pauli_pass_args(p, 1ull << n);
        if (!pass.ok) return qsv_fail(QSV_EINVAL, "bad Pauli pass");
        const int item_bits = p.pivot < 0 ? n : n - 1;
        const EnsArgs e = ens_args(n, members, item_bits, part_bits(item_bits, st->grid_cap));
        launches.push_back({pass, e});
        offsets->push_back(doubles);
        widths->push_back(pass.width);
        doubles += static_cast<size_t>(members) * pass.width;
        most_partials = std::max(most_partials, (static_cast<size_t>(members) << e.part_bits) * pass.width);
    }
    int rc = qsvk_ensure_matrix(st, sizeof(double) * (doubles + most_partials));
    if (rc) return rc;
    double *values = st->dev_matrix, *partials = st->dev_matrix + doubles;
    for (size_t k = 0; k < passes.size(); ++k) {
        const Launch &l = launches[k];
        with_pow2<1, 8>(l.pass.width, [&](auto W) { with_bool(passes[k].pivot < 0, [&](auto DIAG) {
            hipLaunchKernelGGL((k_ens_expect_pauli_group<W.value, DIAG.value>), dim3(ens_grid(l.e, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                               static_cast<const amp_t *>(st->data), l.pass.g, l.e, partials);
        }); });
        rc = check_launch();
        if (rc) return rc;
        const uint64_t count = members * l.pass.width;
        hipLaunchKernelGGL(k_ens_sum_parts, dim3(grid_for(count, QSV_BLOCK, QSV_REDUCE_BLOCKS)), dim3(QSV_BLOCK), 0, st->stream,
                           static_cast<const double *>(partials), members, 1 << l.e.part_bits, l.pass.width, values + (*offsets)[k]);
        rc = check_launch();
        if (rc) return rc;
    }
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_expect_pauli_group");
    host->assign(doubles, 0.0);
    QSV_HIP(hipMemcpyAsync(host->data(), values, sizeof(double) * doubles, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

}  // namespace

// k_ens_sum_parts for the ensemble kernels of other translation units (qsv_sweep.hip): on st's stream, no synchronisation
int qsvk_ens_sum_parts(qsv_state *st, const double *partials, uint64_t members, int parts, int R, double *out) {
    hipLaunchKernelGGL(k_ens_sum_parts, dim3(grid_for(members * R, QSV_BLOCK, QSV_REDUCE_BLOCKS)), dim3(QSV_BLOCK), 0, st->stream, partials, members,
                       parts, R, out);
    return check_launch();
}

// What the ensemble calls of other translation units (qsv_ensemble_adjoint.hip) need of the register's workspace.
// qsvk_ens_check_member_size: the refusal of check_member_size, before anything is flushed; allocates nothing.
int qsvk_ens_check_member_size(qsv_state *st, int n) {
    if (!st->ensemble_work) return QSV_OK;
    return check_member_size(static_cast<const EnsembleWork *>(st->ensemble_work), n, st->amps >> n);
}
// The workspace sized for members of n qubits: *partials = its [members][P_max(n)][16] doubles, *slots = its [members][32].
int qsvk_ens_workspace(qsv_state *st, int n, double **partials, double **slots) {
    EnsembleWork *work = work_of(st);
    const int rc = ensure_workspace(st, work, n, st->amps >> n);
    if (rc) return rc;
    *partials = work->dev + work->ws.partials;
    *slots = work->dev + work->ws.matrix;
    return QSV_OK;
}

extern "C" {

int qsv_ensemble_broadcast(qsv_state *st, int member_qubits) {
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    // the filled part doubles with every copy; source and destination never meet
    for (uint64_t filled = 1ull << member_qubits; filled < st->amps; filled *= 2) {
        rc = qsvk_copy(st->data + filled, st->data, filled, st->stream);
        if (rc) return rc;
    }
    return QSV_OK;
}

int qsv_ensemble_apply_channel(qsv_state *st, int member_qubits, qsv_channel *c, const int *qubits, const double *u01, const int *forced) {
    if (!st || !c || !qubits || !u01) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, c->k);
    if (rc) return rc;
    if (st->device != c->device) return qsv_fail(QSV_EINVAL, "register and channel on different devices");
    rc = check_member_qubits(member_qubits, c->k, qubits);
    if (rc) return rc;
    const int n = member_qubits;
    const uint64_t members = st->amps >> n;
    for (uint64_t m = 0; m < members; ++m) {
        if (!(u01[m] >= 0.0 && u01[m] < 1.0)) return qsv_fail(QSV_EINVAL, "every draw must lie in [0, 1)");
        if (forced && (forced[m] < -1 || forced[m] >= c->n_kraus)) return qsv_fail(QSV_EINVAL, "forced branch out of range");
    }
    EnsembleWork *work = work_of(st);
    if (work->dev && (work->n != n || work->ws.members != members) && pending_steps(work) > 0)
        return qsv_fail(QSV_ESTATE, "read the ensemble log before changing the member size");
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_workspace(st, work, n, members);
    if (rc) return rc;
    if (work->used == work->ws.slots) {
        rc = drain(st, work);
        if (rc) return rc;
    }
    // the draws: the ring slot of this step's log slot, which the drain above (or the log read) has made free
    double *slot = work->ring + 2 * members * static_cast<size_t>(work->used);
    for (uint64_t m = 0; m < members; ++m) {
        slot[2 * m] = u01[m];
        slot[2 * m + 1] = forced ? static_cast<double>(forced[m]) : -1.0;
    }
    double *partials = work->dev + work->ws.partials, *matrix = work->dev + work->ws.matrix, *draws = work->dev + work->ws.draws;
    double *log = work->dev + work->ws.log + 2 * members * static_cast<size_t>(work->used);
    QSV_HIP(hipMemcpyAsync(draws, slot, sizeof(double) * 2 * members, hipMemcpyHostToDevice, st->stream));
    int bits[2] = {0, 0};
    for (int i = 0; i < c->k; ++i) bits[i] = n - 1 - qubits[i];
    const ChannelPlan plan = ens_channel_plan(n, c->k, bits, ens_lanes(n, st->readout_variant != 1));
    const bool nt = st->nontemporal != 0;
    const int item_bits = n - plan.kh;
    const EnsArgs read = ens_args(n, members, item_bits, part_bits(item_bits, st->grid_cap));
    const EnsArgs update = ens_args(n, members, item_bits, apply_part_bits(item_bits, st->grid_cap));
    if (!c->mixed_unitary) {
        with_shape(plan.k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
            hipLaunchKernelGGL((k_ens_channel_rdm<K.value, KL.value, NT.value>), dim3(ens_grid(read, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                               static_cast<const amp_t *>(st->data), plan.g, read, partials);
        });
        rc = check_launch();
        if (rc) return rc;
    }
    const uint64_t select_blocks = (members + QSV_BLOCK / ENS_SELECT_LANES - 1) / (QSV_BLOCK / ENS_SELECT_LANES);
    hipLaunchKernelGGL(k_ens_channel_select, dim3(static_cast<unsigned>(std::min<uint64_t>(select_blocks, CH_MAX_BLOCKS))), dim3(QSV_BLOCK), 0, st->stream,
                       static_cast<const double *>(partials), 1 << read.part_bits, static_cast<const double *>(c->dev), c->n_kraus, c->D,
                       c->mixed_unitary ? 1 : 0, static_cast<const double *>(draws), members, matrix, log);
    rc = check_launch();
    if (rc) return rc;
    ++work->used;     // the log slot is written from here on, whatever becomes of the update pass
    with_shape(plan.k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_ens_channel_apply<K.value, KL.value, NT.value>), dim3(ens_grid(update, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           st->data, plan.g, update, static_cast<const double *>(matrix));
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_channel_apply<%d, %d, %s>%s", plan.k, plan.kl, nt ? "true" : "false",
             c->mixed_unitary ? " after k_ens_channel_select" : " after k_ens_channel_rdm");
    return check_launch();
}

int qsv_ensemble_log_read(qsv_state *st, int32_t *branches, double *probs, uint64_t capacity_steps, uint64_t *steps) {
    if (!st || !steps) return qsv_fail(QSV_EINVAL, "null pointer");
    if (capacity_steps && (!branches || !probs)) return qsv_fail(QSV_EINVAL, "null pointer");
    EnsembleWork *work = static_cast<EnsembleWork *>(st->ensemble_work);
    const uint64_t pending = work ? pending_steps(work) : 0;
    *steps = pending;
    if (pending == 0 || capacity_steps < pending) return QSV_OK;
    QSV_HIP(hipSetDevice(st->device));
    QSV_HIP(hipStreamSynchronize(st->stream));
    const int rc = drain(st, work);
    if (rc) return rc;
    std::memcpy(branches, work->branches.data(), sizeof(int32_t) * work->branches.size());
    std::memcpy(probs, work->probs.data(), sizeof(double) * work->probs.size());
    work->branches.clear();
    work->probs.clear();
    return QSV_OK;
}

int qsv_ensemble_measure(qsv_state *st, int member_qubits, int qubit, const double eig0[4], const double eig1[4], int after, int bit,
                         const double *u01, const int *forced) {
    if (!st || !eig0 || !eig1 || !u01) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 1);
    if (rc) return rc;
    rc = check_member_qubits(member_qubits, 1, &qubit);
    if (rc) return rc;
    if (after < 0 || after > 1) return qsv_fail(QSV_EINVAL, "after is 0 (keep the eigenvector) or 1 (reset to |0>)");
    if (bit < -1 || bit > 63) return qsv_fail(QSV_EINVAL, "a member has the classical bits 0 .. 63 (-1: none)");
    const int n = member_qubits;
    const uint64_t members = st->amps >> n;
    for (uint64_t m = 0; m < members; ++m) {
        if (!(u01[m] >= 0.0 && u01[m] < 1.0)) return qsv_fail(QSV_EINVAL, "every draw must lie in [0, 1)");
        if (forced && (forced[m] < -1 || forced[m] > 1)) return qsv_fail(QSV_EINVAL, "forced outcome out of range");
    }
    EnsembleWork *work = work_of(st);
    rc = check_member_size(work, n, members);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_workspace(st, work, n, members);
    if (rc) return rc;
    rc = ensure_bits(st, work, n, members);
    if (rc) return rc;
    if (work->used == work->ws.slots) {
        rc = drain(st, work);
        if (rc) return rc;
    }
    double *slot = work->ring + 2 * members * static_cast<size_t>(work->used);
    for (uint64_t m = 0; m < members; ++m) {
        slot[2 * m] = u01[m];
        slot[2 * m + 1] = forced ? static_cast<double>(forced[m]) : -1.0;
    }
    double *partials = work->dev + work->ws.partials, *matrix = work->dev + work->ws.matrix, *draws = work->dev + work->ws.draws;
    double *log = work->dev + work->ws.log + 2 * members * static_cast<size_t>(work->used);
    QSV_HIP(hipMemcpyAsync(draws, slot, sizeof(double) * 2 * members, hipMemcpyHostToDevice, st->stream));
    const int bits[2] = {n - 1 - qubit, 0};
    const ChannelPlan plan = ens_channel_plan(n, 1, bits, ens_lanes(n, st->readout_variant != 1));
    const bool nt = st->nontemporal != 0;
    const int item_bits = n - plan.kh;
    const EnsArgs read = ens_args(n, members, item_bits, part_bits(item_bits, st->grid_cap));
    const EnsArgs update = ens_args(n, members, item_bits, apply_part_bits(item_bits, st->grid_cap));
    MeasureArgs args;
    std::memcpy(args.eig[0], eig0, sizeof(double) * 4);
    std::memcpy(args.eig[1], eig1, sizeof(double) * 4);
    args.after = after;
    args.bit = bit;
    with_shape(1, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_ens_channel_rdm<K.value, KL.value, NT.value>), dim3(ens_grid(read, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           static_cast<const amp_t *>(st->data), plan.g, read, partials);
    });
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_ens_measure_select, dim3(grid_for(members, QSV_BLOCK, static_cast<int>(CH_MAX_BLOCKS))), dim3(QSV_BLOCK), 0, st->stream,
                       static_cast<const double *>(partials), 1 << read.part_bits, args, static_cast<const double *>(draws), members, matrix, log,
                       work->bits);
    rc = check_launch();
    if (rc) return rc;
    ++work->used;     // the log slot is written from here on, whatever becomes of the update pass
    with_shape(1, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_ens_channel_apply<K.value, KL.value, NT.value>), dim3(ens_grid(update, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           st->data, plan.g, update, static_cast<const double *>(matrix));
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_channel_apply<1, %d, %s> after k_ens_measure_select after k_ens_channel_rdm", plan.kl,
             nt ? "true" : "false");
    return check_launch();
}

int qsv_ensemble_apply_conditional(qsv_state *st, int member_qubits, int k, const int *qubits, const double *matrix, uint64_t all_of,
                                   uint64_t none_of) {
    if (!st || !qubits || !matrix) return qsv_fail(QSV_EINVAL, "null pointer");
    if (k < 1 || k > 2) return qsv_fail(QSV_EINVAL, "a conditional gate acts on 1 or 2 qubits");
    int rc = check_ensemble(st, member_qubits, k);
    if (rc) return rc;
    rc = check_member_qubits(member_qubits, k, qubits);
    if (rc) return rc;
    if (!qsv_ensemble_control_layout::masks_ok(all_of, none_of)) return qsv_fail(QSV_EINVAL, "a bit cannot be asked to be both set and clear");
    const int n = member_qubits;
    const uint64_t members = st->amps >> n;
    EnsembleWork *work = work_of(st);
    rc = check_member_size(work, n, members);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_bits(st, work, n, members);
    if (rc) return rc;
    int bits[2] = {0, 0};
    for (int i = 0; i < k; ++i) bits[i] = n - 1 - qubits[i];
    const ChannelPlan plan = ens_channel_plan(n, k, bits, ens_lanes(n, st->readout_variant != 1));
    const bool nt = st->nontemporal != 0;
    const int item_bits = n - plan.kh;
    const EnsArgs update = ens_args(n, members, item_bits, apply_part_bits(item_bits, st->grid_cap));
    ConditionalArgs args;
    std::memset(&args, 0, sizeof(args));
    std::memcpy(args.m, matrix, sizeof(double) * 2 * (size_t(1) << (2 * k)));
    args.all_of = all_of;
    args.none_of = none_of;
    args.chunk_bits = qsv_ensemble_control_layout::cond_unit_uniform(update) ? qsv_ensemble_control_layout::cond_chunk_bits(update.units) : 0;
    with_shape(k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_ens_apply_conditional<K.value, KL.value, NT.value>), dim3(cond_grid(update, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           st->data, plan.g, update, args, static_cast<const uint64_t *>(work->bits));
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_apply_conditional<%d, %d, %s>", k, plan.kl, nt ? "true" : "false");
    return check_launch();
}

// Every member its own matrix: the update pass of a channel call with the matrix slots filled by the caller instead of by
// k_ens_channel_select.  Nothing is drawn, nothing is logged.  The slots belong to the register's stream: the copy below is
// queued behind the update pass of any earlier step that still reads them.
int qsv_ensemble_apply_matrices(qsv_state *st, int member_qubits, int k, const int *qubits, const double *matrices) {
    if (!st || !qubits || !matrices) return qsv_fail(QSV_EINVAL, "null pointer");
    if (k < 1 || k > 2) return qsv_fail(QSV_EINVAL, "per-member matrices act on 1 or 2 qubits");
    int rc = check_ensemble(st, member_qubits, k);
    if (rc) return rc;
    rc = check_member_qubits(member_qubits, k, qubits);
    if (rc) return rc;
    const int n = member_qubits;
    const uint64_t members = st->amps >> n;
    const size_t entries = size_t(2) << (2 * k);     // doubles of one matrix
    for (size_t i = 0; i < members * entries; ++i)
        if (!std::isfinite(matrices[i])) return qsv_fail(QSV_EINVAL, "every matrix entry must be finite");
    EnsembleWork *work = work_of(st);
    rc = check_member_size(work, n, members);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_workspace(st, work, n, members);
    if (rc) return rc;
    std::vector<double> slots(static_cast<size_t>(members) * 32, 0.0);
    for (uint64_t m = 0; m < members; ++m) std::memcpy(&slots[32 * m], matrices + m * entries, sizeof(double) * entries);
    double *matrix = work->dev + work->ws.matrix;
    // pageable memory: the copy has left `slots` when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(matrix, slots.data(), sizeof(double) * slots.size(), hipMemcpyHostToDevice, st->stream));
    int bits[2] = {0, 0};
    for (int i = 0; i < k; ++i) bits[i] = n - 1 - qubits[i];
    const ChannelPlan plan = ens_channel_plan(n, k, bits, ens_lanes(n, st->readout_variant != 1));
    const bool nt = st->nontemporal != 0;
    const int item_bits = n - plan.kh;
    const EnsArgs update = ens_args(n, members, item_bits, apply_part_bits(item_bits, st->grid_cap));
    with_shape(plan.k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_ens_channel_apply<K.value, KL.value, NT.value>), dim3(ens_grid(update, st->grid_cap)), dim3(QSV_BLOCK), 0, st->stream,
                           st->data, plan.g, update, static_cast<const double *>(matrix));
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_ens_channel_apply<%d, %d, %s>", plan.k, plan.kl, nt ? "true" : "false");
    return check_launch();
}

int qsv_ensemble_bits_read(qsv_state *st, int member_qubits, uint64_t *bits) {
    if (!st || !bits) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    const uint64_t members = st->amps >> member_qubits;
    EnsembleWork *work = work_of(st);
    rc = check_member_size(work, member_qubits, members);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_bits(st, work, member_qubits, members);
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(bits, work->bits, qsv_ensemble_control_layout::bits_bytes(members), hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

int qsv_ensemble_bits_write(qsv_state *st, int member_qubits, const uint64_t *bits) {
    if (!st) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    const uint64_t members = st->amps >> member_qubits;
    EnsembleWork *work = work_of(st);
    rc = check_member_size(work, member_qubits, members);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_bits(st, work, member_qubits, members);
    if (rc) return rc;
    if (!bits) {
        QSV_HIP(hipMemsetAsync(work->bits, 0, qsv_ensemble_control_layout::bits_bytes(members), st->stream));
        return QSV_OK;
    }
    // pageable memory: the copy has left the caller's buffer when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(work->bits, bits, qsv_ensemble_control_layout::bits_bytes(members), hipMemcpyHostToDevice, st->stream));
    return QSV_OK;
}

int qsv_ensemble_norm2(qsv_state *st, int member_qubits, double *out) {
    if (!st || !out) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 1);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    // the diagonal pass with a zero zmask: sum |psi_i|^2 per member
    std::vector<qsv_pauli_plan::Pass> plan(1);
    plan[0].zmask.push_back(0);
    plan[0].n_y.push_back(0);
    plan[0].index.push_back(0);
    std::vector<double> host;
    std::vector<size_t> offsets;
    std::vector<int> widths;
    rc = expect_passes(st, member_qubits, plan, &host, &offsets, &widths);
    if (rc) return rc;
    const uint64_t members = st->amps >> member_qubits;
    for (uint64_t m = 0; m < members; ++m) out[m] = host[m * widths[0]];
    return QSV_OK;
}

int qsv_ensemble_expect_pauli_sum(qsv_state *st, int member_qubits, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                                  const double *coeffs, double *values, double *term_values) {
    if (!st || !values) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_terms < 0) return qsv_fail(QSV_EINVAL, "negative number of Pauli terms");
    if (n_terms > 0 && !term_offsets) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_ensemble(st, member_qubits, 1);
    if (rc) return rc;
    // the whole list is checked and turned into masks of member bits before anything is flushed or launched
    const int n = member_qubits;
    std::vector<qsv_pauli_plan::Term> terms;
    rc = parse_member_terms(n, n_terms, term_offsets, qubits, paulis, &terms);
    if (rc) return rc;
    const uint64_t members = st->amps >> n;
    for (uint64_t m = 0; m < members; ++m) values[m] = 0.0;
    if (n_terms == 0) return QSV_OK;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    const std::vector<qsv_pauli_plan::Pass> plan = qsv_pauli_plan::plan(terms);
    std::vector<double> host;
    std::vector<size_t> offsets;
    std::vector<int> widths;
    rc = expect_passes(st, n, plan, &host, &offsets, &widths);
    if (rc) return rc;
    std::vector<double> per_term(static_cast<size_t>(n_terms));
    for (uint64_t m = 0; m < members; ++m) {
        for (size_t k = 0; k < plan.size(); ++k) {
            const qsv_pauli_plan::Pass &p = plan[k];
            for (size_t t = 0; t < p.zmask.size(); ++t)
                per_term[p.index[t]] = qsv_pauli_plan::pair_scale(p.pivot, p.n_y[t]) * host[offsets[k] + m * widths[k] + t];
        }
        double sum = 0.0;
        for (int t = 0; t < n_terms; ++t) {     // in the caller's order
            sum += (coeffs ? coeffs[t] : 1.0) * per_term[t];
            if (term_values) term_values[m * n_terms + t] = per_term[t];
        }
        values[m] = sum;
    }
    return QSV_OK;
}

}  // extern "C"

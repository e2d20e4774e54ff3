// Kraus channels on kets (quantum trajectories) and Pauli traces of density registers (gfx950, wave64) with their C entry
// points.  A general channel call is two passes over the register and no host synchronisation:
//   k_channel_rdm     reads the register once and leaves the 2^k x 2^k reduced density matrix of the target qubits as
//                     real partial sums per workgroup; k_sum_partials (qsv_readout.hip) adds them on the device;
//   k_channel_select  one workgroup: branch weights w_j = Re tr(E_j rho), the choice, the chosen K_j sqrt(total / w_j) into
//                     a device matrix slot and (j, w_j / total) into the register's device log;
//   k_channel_apply   one in-place pass with the matrix it finds in that slot.
// The choice is made in ONE place and every workgroup of the update pass reads its outcome: they cannot disagree.
// Streaming style of k_measure_probs_s / k_collapse_s: a work item is 64 consecutive amplitudes per wave instruction, every
// global access a whole 1 KiB segment, a target bit below 6 is resolved with shfl_xor.  Launch shapes: qsv_channel_layout.h.

#include "qsv_device.h"
#include "qsv_channel_layout.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

using namespace qsv_channel_layout;

static_assert(CH_BLOCK == QSV_BLOCK && CH_REDUCE_BLOCKS == QSV_REDUCE_BLOCKS && CH_LANE_BITS == QSV_LANE_BITS &&
              CH_MIN_STREAM_QUBITS == qsv_readout_layout::RO_MIN_QUBITS, "qsv_channel_layout.h mirrors qsv_internal.h");

namespace {

// A register's channel workspace (device) and its branch log.  Entries are kept in call order; an entry whose branch was
// chosen on the device holds the device slot its numbers will be found in until the slots are drained.
struct ChannelWork {
    int device = 0;
    double *dev = nullptr;            // WS_DOUBLES doubles
    int used = 0;                     // device log slots written since the last drain
    std::vector<int32_t> branches;
    std::vector<double> probs;
    std::vector<int> slot;            // -1: chosen on the host, numbers already in place
};

void free_work(void *p) {
    ChannelWork *w = static_cast<ChannelWork *>(p);
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->dev) (void)hipFree(w->dev);
    delete w;
}

int ensure_work(qsv_state *st, ChannelWork **out) {
    if (!st->channel_work) {
        ChannelWork *w = new ChannelWork;
        w->device = st->device;
        st->channel_work = w;
        st->channel_work_free = free_work;
    }
    *out = static_cast<ChannelWork *>(st->channel_work);
    return QSV_OK;
}

int ensure_device_work(ChannelWork *w) {
    if (w->dev) return QSV_OK;
    if (hipMalloc(reinterpret_cast<void **>(&w->dev), sizeof(double) * WS_DOUBLES) != hipSuccess)
        return qsv_fail(QSV_ENOMEM, "device allocation of the channel workspace failed");
    return QSV_OK;
}

// Device log -> host entries.  One copy and one synchronisation; the only time qsv_apply_channel may wait.
int drain(qsv_state *st, ChannelWork *w) {
    if (w->used == 0) return QSV_OK;
    std::vector<double> host(2 * static_cast<size_t>(w->used));
    QSV_HIP(hipMemcpyAsync(host.data(), w->dev + WS_LOG, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    for (size_t e = 0; e < w->slot.size(); ++e) {
        const int s = w->slot[e];
        if (s < 0) continue;
        w->branches[e] = static_cast<int32_t>(host[2 * s]);
        w->probs[e] = host[2 * s + 1];
        w->slot[e] = -1;
    }
    w->used = 0;
    return QSV_OK;
}

// x conj(y)
__device__ __forceinline__ amp_t mul_conj(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.y, y.x, -(x.x * y.y))};
}

// what a low combination adds to the group index: glo[] is linear under OR, so two selects serve a per-lane l
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

// The workgroup's sums of R doubles per thread -> partials[block * R + e]: wave shuffle, LDS, one partial per slot.
template <int R>
__device__ __forceinline__ void block_store_sums(const double (&v)[R], double *__restrict__ partials) {
    __shared__ double sums[QSV_BLOCK / 64][R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const double s = wave_sum(v[e]);
        if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < R) {
        double s = 0.0;
        for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) s += sums[wv][threadIdx.x];
        partials[static_cast<uint64_t>(blockIdx.x) * R + threadIdx.x] = s;
    }
}

// partials[block][D * D] = this workgroup's share of the reduced density matrix of the K target bits, as real numbers
// (rdm_pair_slot).  Read-only.  A thread owns the 2^KH amplitudes x[h] of its item and sees the 2^KL - 1 partner lanes'
// through shfl_xor; it accumulates x[h] conj(partner) under STATIC indices (h, h', dl) and sorts the sums into matrix
// entries once, after the loop.  With partner lanes an entry (r, c) is formed by the owner of r alone, so keeping r <= c
// counts each once; without them (KL = 0) the thread forms each pair once, h <= h', and conjugates where that is r > c.
template <int K, int KL, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_channel_rdm(const amp_t *__restrict__ a, const ChannelArgs g, double *__restrict__ partials) {
    constexpr int KH = K - KL, NH = 1 << KH, NL = 1 << KL, D = 1 << K, R = D * D;
    amp_t acc[NH][NH][NL];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int dl = 0; dl < NL; ++dl) acc[h][j][dl] = amp_t{0.0, 0.0};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    // W is a multiple of 64 whenever KL > 0 (registers of at least 2^14 amplitudes): a wave is in the loop as a whole
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.W; w += stride) {
        const uint64_t base = deposit(w, g);
        amp_t x[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) x[h] = ld<NT>(a + base + g.hoff[h]);
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int dl = 0; dl < NL; ++dl) {
                const amp_t y = dl == 0 ? x[j] : shfl_xor_amp(x[j], g.lxor[dl]);
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    if (KL == 0 && h > j) continue;      // no partner lanes: the thread holds both orders itself
                    const amp_t p = mul_conj(x[h], y);
                    acc[h][j][dl].x += p.x;
                    acc[h][j][dl].y += p.y;
                }
            }
    }
    const int l_own = own_combination<KL>(g);
    double v[R];
#pragma unroll
    for (int e = 0; e < R; ++e) v[e] = 0.0;
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
                if (KL == 0 && r > c) {      // h < j does not order the group indices: the entry below the diagonal, conjugated
                    const int t = r;
                    r = c;
                    c = t;
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
    block_store_sums<R>(v, partials);
}

// One workgroup.  rho: rdm_entries(D) reals; chan: K_0 .. K_{n-1} then E_0 .. E_{n-1}.  Thread j forms w_j; thread 0 adds
// them in index order and takes the branch (pick_branch of qsv_channel_layout.h, step for step); threads e < D * D write
// the scaled matrix; thread 0 writes the log entry.  No division by zero anywhere: a branch of weight 0 gives zeros.
__global__ __launch_bounds__(64) void k_channel_select(const double *__restrict__ rho, const double *__restrict__ chan, int n_kraus, int D,
                                                       double u, int forced, double *__restrict__ matrix, double *__restrict__ log) {
    __shared__ double w[CH_MAX_KRAUS];
    __shared__ int chosen;
    __shared__ double scale;
    const int t = threadIdx.x, DD = D * D;
    if (t < n_kraus) {
        const double *E = chan + 2 * static_cast<size_t>(DD) * (n_kraus + t);
        double s = 0.0;
        for (int r = 0; r < D; ++r) s += E[2 * (r * D + r)] * rho[r];
        int slot = D;
        double off = 0.0;
        for (int r = 0; r < D; ++r)
            for (int c = r + 1; c < D; ++c) {
                // E[r][c] rho[c][r] + its conjugate, rho[c][r] = conj(rho[r][c])
                off += E[2 * (r * D + c)] * rho[slot] + E[2 * (r * D + c) + 1] * rho[slot + 1];
                slot += 2;
            }
        w[t] = s + 2.0 * off;
    }
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int j = 0; j < n_kraus; ++j) total += w[j];
        int pick = forced;
        if (pick < 0) {
            const double target = u * total;
            double run = 0.0;
            int last = -1;
            for (int j = 0; j < n_kraus && pick < 0; ++j) {
                run += w[j];
                if (w[j] > 0.0) last = j;
                if (run > target && w[j] > 0.0) pick = j;
            }
            if (pick < 0) pick = last < 0 ? 0 : last;
        }
        const double wj = w[pick];
        const bool live = wj > 0.0 && total > 0.0;
        chosen = pick;
        scale = live ? sqrt(total / wj) : 0.0;
        log[0] = static_cast<double>(pick);
        log[1] = live ? wj / total : 0.0;
    }
    __syncthreads();
    if (t < DD) {
        const double *Kj = chan + 2 * static_cast<size_t>(DD) * chosen;
        const double s = scale;
        // a scale of 0 writes zeros whatever K_j holds (0 * inf would not)
        matrix[2 * t] = s != 0.0 ? Kj[2 * t] * s : 0.0;
        matrix[2 * t + 1] = s != 0.0 ? Kj[2 * t + 1] * s : 0.0;
    }
}

// a[group] <- M a[group] in place, M the D x D matrix in device memory (row-major, interleaved complex, leg 0 = most
// significant index bit).  Every thread loads all it needs before it stores, and the groups of different waves are
// disjoint, so there is no scratch register.  The matrix entries a lane needs depend on its own low combination only:
// they are fetched once, before the loop.
template <int K, int KL, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_channel_apply(amp_t *__restrict__ a, const ChannelArgs g, const double *__restrict__ m) {
    constexpr int KH = K - KL, NH = 1 << KH, NL = 1 << KL, D = 1 << K;
    const int l_own = own_combination<KL>(g);
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
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; w < g.W; w += stride) {
        const uint64_t base = deposit(w, g);
        amp_t x[NH], out[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            x[h] = ld<NT>(a + base + g.hoff[h]);
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
        for (int h = 0; h < NH; ++h) st<NT>(a + base + g.hoff[h], out[h]);
    }
}

// tr(P_t rho) for one Pauli string per workgroup: P|k> = i^nY (-1)^popcount(k & z) |k ^ x>, so the trace is
// i^nY sum_k (-1)^popcount(k & z) rho[k][k ^ x] -- 2^n entries of the 4^n register.  Sums in a fixed order.
struct DensityTerm {
    uint64_t xmask, zmask;
    int32_t n_y, unused;
};
__global__ __launch_bounds__(QSV_BLOCK) void k_density_expect_paulis(const amp_t *__restrict__ rho, int nbits, const DensityTerm *__restrict__ table,
                                                                     double *__restrict__ out) {
    const DensityTerm term = table[blockIdx.x];
    const uint64_t dim = 1ull << nbits;
    double re = 0.0, im = 0.0;
    for (uint64_t k = threadIdx.x; k < dim; k += QSV_BLOCK) {
        const amp_t v = rho[(k << nbits) | (k ^ term.xmask)];
        const bool minus = __popcll(k & term.zmask) & 1;
        re += minus ? -v.x : v.x;
        im += minus ? -v.y : v.y;
    }
    block_sum2(re, im);
    if (threadIdx.x == 0) {
        double r = re, i = im;
        switch (term.n_y & 3) {
            case 1: r = -im; i = re; break;
            case 2: r = -re; i = -im; break;
            case 3: r = im; i = -re; break;
            default: break;
        }
        out[2 * blockIdx.x] = r;
        out[2 * blockIdx.x + 1] = i;
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

// everything qsv_apply_channel refuses, before any launch and with the queue untouched
int check_call(const qsv_state *st, const qsv_channel *c, const int *qubits, double u01, int forced) {
    if (!st || !c || !qubits) return qsv_fail(QSV_EINVAL, "null pointer");
    if (st->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs a qubit register");
    if (st->device != c->device) return qsv_fail(QSV_EINVAL, "register and channel on different devices");
    for (int i = 0; i < c->k; ++i) {
        if (qubits[i] < 0) return qsv_fail(QSV_EINVAL, "Non-negative index");
        if (qubits[i] >= st->n)
            return qsv_fail(QSV_EINVAL, "qubit index " + std::to_string(qubits[i]) + " out of range for a " + std::to_string(st->n) +
                                            "-qubit register");
        for (int j = 0; j < i; ++j)
            if (qubits[i] == qubits[j]) return qsv_fail(QSV_EINVAL, "Indices must be distinct.");
    }
    if (!(u01 >= 0.0 && u01 < 1.0)) return qsv_fail(QSV_EINVAL, "the draw must lie in [0, 1)");
    if (forced < -1 || forced >= c->n_kraus) return qsv_fail(QSV_EINVAL, "forced branch out of range");
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_channel_create(int k, int n_kraus, const double *kraus, int device, qsv_channel **out) {
    if (!out) return qsv_fail(QSV_EINVAL, "null pointer");
    *out = nullptr;
    if (!kraus) return qsv_fail(QSV_EINVAL, "null pointer");
    if (k != 1 && k != 2) return qsv_fail(QSV_EINVAL, "a channel acts on 1 or 2 qubits");
    if (n_kraus < 1 || n_kraus > CH_MAX_KRAUS) return qsv_fail(QSV_EINVAL, "a channel has 1 to 16 Kraus operators");
    const int D = 1 << k, DD = D * D;
    for (int i = 0; i < 2 * DD * n_kraus; ++i)
        if (!std::isfinite(kraus[i])) return qsv_fail(QSV_EINVAL, "Kraus operators must be finite");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return qsv_fail(QSV_EHIP, "no HIP device");
    if (device < 0 || device >= count) return qsv_fail(QSV_EINVAL, "no such device");
    QSV_HIP(hipSetDevice(device));
    // E_j = K_j^dagger K_j
    std::vector<double> table(4 * static_cast<size_t>(DD) * n_kraus, 0.0);
    std::memcpy(table.data(), kraus, sizeof(double) * 2 * DD * n_kraus);
    double *E = table.data() + 2 * static_cast<size_t>(DD) * n_kraus;
    for (int j = 0; j < n_kraus; ++j) {
        const double *K = kraus + 2 * static_cast<size_t>(DD) * j;
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) {
                double re = 0.0, im = 0.0;
                for (int r = 0; r < D; ++r) {   // conj(K[r][a]) K[r][b]
                    const double xr = K[2 * (r * D + a)], xi = K[2 * (r * D + a) + 1], yr = K[2 * (r * D + b)], yi = K[2 * (r * D + b) + 1];
                    re += xr * yr + xi * yi;
                    im += xr * yi - xi * yr;
                }
                E[2 * (static_cast<size_t>(DD) * j + a * D + b)] = re;
                E[2 * (static_cast<size_t>(DD) * j + a * D + b) + 1] = im;
            }
    }
    qsv_channel *c = new qsv_channel;
    c->device = device;
    c->k = k;
    c->D = D;
    c->n_kraus = n_kraus;
    // mixed-unitary: every E_j is p_j I to 16 eps per entry
    const double tol = 16.0 * std::numeric_limits<double>::epsilon();
    c->mixed_unitary = true;
    c->p.assign(n_kraus, 0.0);
    for (int j = 0; j < n_kraus && c->mixed_unitary; ++j) {
        const double *Ej = E + 2 * static_cast<size_t>(DD) * j;
        const double pj = Ej[0];
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) {
                const double want = a == b ? pj : 0.0;
                if (std::fabs(Ej[2 * (a * D + b)] - want) > tol || std::fabs(Ej[2 * (a * D + b) + 1]) > tol) c->mixed_unitary = false;
            }
        c->p[j] = pj;
    }
    if (c->mixed_unitary) {
        c->unitaries.assign(2 * static_cast<size_t>(DD) * n_kraus, 0.0);
        for (int j = 0; j < n_kraus; ++j) {
            if (!(c->p[j] > 0.0)) continue;
            const double root = std::sqrt(c->p[j]);
            for (int e = 0; e < 2 * DD; ++e) c->unitaries[2 * static_cast<size_t>(DD) * j + e] = kraus[2 * static_cast<size_t>(DD) * j + e] / root;
        }
    }
    const size_t bytes = sizeof(double) * table.size();
    if (hipMalloc(reinterpret_cast<void **>(&c->dev), bytes) != hipSuccess) {
        delete c;
        return qsv_fail(QSV_ENOMEM, "device allocation of the channel failed");
    }
    hipError_t e = hipMemcpy(c->dev, table.data(), bytes, hipMemcpyHostToDevice);   // the table dies at return
    if (e != hipSuccess) {
        (void)hipFree(c->dev);
        delete c;
        return qsv_fail(QSV_EHIP, std::string("upload of the channel: ") + hipGetErrorString(e));
    }
    *out = c;
    return QSV_OK;
}

int qsv_channel_destroy(qsv_channel *c) {
    if (!c) return QSV_OK;
    (void)hipSetDevice(c->device);
    if (c->dev) (void)hipFree(c->dev);
    delete c;
    return QSV_OK;
}

int qsv_channel_info(const qsv_channel *c, int *k, int *n_kraus, int *mixed_unitary) {
    if (!c) return qsv_fail(QSV_EINVAL, "null channel");
    if (k) *k = c->k;
    if (n_kraus) *n_kraus = c->n_kraus;
    if (mixed_unitary) *mixed_unitary = c->mixed_unitary ? 1 : 0;
    return QSV_OK;
}

int qsv_apply_channel(qsv_state *st, qsv_channel *c, const int *qubits, double u01, int forced) {
    int rc = check_call(st, c, qubits, u01, forced);
    if (rc) return rc;
    ChannelWork *work = nullptr;
    rc = ensure_work(st, &work);
    if (rc) return rc;
    const int DD = c->D * c->D;
    if (c->mixed_unitary) {
        // the weights do not depend on the state: the host picks, and the gate joins the deferred queue like any other
        double total = 0.0;
        const int drawn = pick_branch(c->p.data(), c->n_kraus, u01, &total);
        const int j = forced >= 0 ? forced : drawn;
        const double *U = c->unitaries.data() + 2 * static_cast<size_t>(DD) * j;
        rc = c->k == 1 ? qsv_apply_1q(st, qubits[0], U) : qsv_apply_2q(st, qubits[0], qubits[1], U);
        if (rc) return rc;
        work->branches.push_back(j);
        work->probs.push_back(c->p[j] > 0.0 && total > 0.0 ? c->p[j] / total : 0.0);
        work->slot.push_back(-1);
        return QSV_OK;
    }
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = ensure_device_work(work);
    if (rc) return rc;
    if (work->used == CH_LOG_SLOTS) {
        rc = drain(st, work);
        if (rc) return rc;
    }
    int bits[2] = {0, 0};
    for (int i = 0; i < c->k; ++i) bits[i] = st->n - 1 - qubits[i];
    const ChannelPlan plan = channel_plan(st->n, st->amps, c->k, bits, streaming_forms(st));
    const bool nt = st->nontemporal != 0;
    const int R = rdm_entries(plan.D), grid_r = rdm_grid(plan.g.W, st->grid_cap), grid_a = apply_grid(plan.g.W, st->grid_cap);
    double *partials = work->dev + WS_PARTIALS, *rho = work->dev + WS_RHO, *matrix = work->dev + WS_MATRIX;
    double *log = work->dev + WS_LOG + 2 * static_cast<size_t>(work->used);
    with_shape(plan.k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_channel_rdm<K.value, KL.value, NT.value>), dim3(grid_r), dim3(QSV_BLOCK), 0, st->stream,
                           static_cast<const amp_t *>(st->data), plan.g, partials);
    });
    rc = check_launch();
    if (rc) return rc;
    rc = qsvk_sum_partials(st->stream, partials, grid_r, R, rho);
    if (rc) return rc;
    hipLaunchKernelGGL(k_channel_select, dim3(1), dim3(64), 0, st->stream, static_cast<const double *>(rho), static_cast<const double *>(c->dev),
                       c->n_kraus, c->D, u01, forced, matrix, log);
    rc = check_launch();
    if (rc) return rc;
    // the log slot is written from here on, whatever becomes of the update pass
    work->branches.push_back(-1);
    work->probs.push_back(0.0);
    work->slot.push_back(work->used++);
    with_shape(plan.k, plan.kl, nt, [&](auto K, auto KL, auto NT) {
        hipLaunchKernelGGL((k_channel_apply<K.value, KL.value, NT.value>), dim3(grid_a), dim3(QSV_BLOCK), 0, st->stream, st->data, plan.g,
                           static_cast<const double *>(matrix));
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_channel_apply<%d, %d, %s>", plan.k, plan.kl, nt ? "true" : "false");
    return check_launch();
}

int qsv_channel_log_read(qsv_state *st, int32_t *branches, double *probs, uint64_t capacity, uint64_t *count) {
    if (!st || !count) return qsv_fail(QSV_EINVAL, "null pointer");
    if (capacity && (!branches || !probs)) return qsv_fail(QSV_EINVAL, "null pointer");
    ChannelWork *work = static_cast<ChannelWork *>(st->channel_work);
    const uint64_t pending = work ? work->branches.size() : 0;
    *count = pending;
    if (pending == 0 || capacity < pending) return QSV_OK;
    QSV_HIP(hipSetDevice(st->device));
    QSV_HIP(hipStreamSynchronize(st->stream));
    const int rc = drain(st, work);
    if (rc) return rc;
    std::memcpy(branches, work->branches.data(), sizeof(int32_t) * pending);
    std::memcpy(probs, work->probs.data(), sizeof(double) * pending);
    work->branches.clear();
    work->probs.clear();
    work->slot.clear();
    return QSV_OK;
}

int qsv_density_expect_paulis(qsv_state *rho, int n_terms, const int *term_offsets, const int *qubits, const char *paulis, double *values) {
    if (!rho) return qsv_fail(QSV_EINVAL, "null pointer");
    if (rho->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs a qubit register");
    if (rho->n & 1) return qsv_fail(QSV_EINVAL, "a density register has an even number of qubits");
    if (n_terms < 0) return qsv_fail(QSV_EINVAL, "negative number of terms");
    if (n_terms > 0 && (!term_offsets || !values)) return qsv_fail(QSV_EINVAL, "null pointer");
    if (n_terms > 0 && term_offsets[0] != 0) return qsv_fail(QSV_EINVAL, "term offsets must start at 0 and not decrease");
    const int n = rho->n / 2;
    std::vector<DensityTerm> table(static_cast<size_t>(n_terms));
    for (int t = 0; t < n_terms; ++t) {
        const int first = term_offsets[t], len = term_offsets[t + 1] - first;
        if (first < 0 || len < 0) return qsv_fail(QSV_EINVAL, "term offsets must start at 0 and not decrease");
        if (len > 64) return qsv_fail(QSV_EINVAL, "bad Pauli string length");
        if (len > 0 && (!qubits || !paulis)) return qsv_fail(QSV_EINVAL, "null pointer");
        DensityTerm row = {0, 0, 0, 0};
        uint64_t seen = 0;
        for (int j = first; j < first + len; ++j) {
            const int q = qubits[j];
            if (q < 0 || q >= n) return qsv_fail(QSV_EINVAL, "qubit index out of range for the density register");
            const uint64_t bit = 1ull << (n - 1 - q);
            if (seen & bit) return qsv_fail(QSV_EINVAL, "Indices must be distinct.");
            seen |= bit;
            switch (paulis[j]) {
                case 'I': case 'i': break;
                case 'X': case 'x': row.xmask |= bit; break;
                case 'Y': case 'y': row.xmask |= bit; row.zmask |= bit; ++row.n_y; break;
                case 'Z': case 'z': row.zmask |= bit; break;
                default: return qsv_fail(QSV_EINVAL, "Pauli letters must be I, X, Y or Z");
            }
        }
        table[t] = row;
    }
    int rc = qsv_flush(rho);
    if (rc) return rc;
    if (n_terms == 0) return QSV_OK;
    QSV_HIP(hipSetDevice(rho->device));
    const size_t b_table = qsv_pad16(sizeof(DensityTerm) * table.size()), b_out = sizeof(double) * 2 * table.size();
    rc = qsvk_ensure_matrix(rho, b_table + b_out);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(rho->dev_matrix);
    DensityTerm *d_table = reinterpret_cast<DensityTerm *>(base);
    double *d_out = reinterpret_cast<double *>(base + b_table);
    QSV_HIP(hipMemcpyAsync(d_table, table.data(), sizeof(DensityTerm) * table.size(), hipMemcpyHostToDevice, rho->stream));
    hipLaunchKernelGGL(k_density_expect_paulis, dim3(n_terms), dim3(QSV_BLOCK), 0, rho->stream, static_cast<const amp_t *>(rho->data), n,
                       static_cast<const DensityTerm *>(d_table), d_out);
    snprintf(rho->last_kernel, sizeof(rho->last_kernel), "k_density_expect_paulis");
    rc = check_launch();
    if (rc) {
        (void)hipStreamSynchronize(rho->stream);   // the upload reads the table
        return rc;
    }
    QSV_HIP(hipMemcpyAsync(values, d_out, b_out, hipMemcpyDeviceToHost, rho->stream));
    QSV_HIP(hipStreamSynchronize(rho->stream));
    return QSV_OK;
}

}  // extern "C"

// The quantum Fourier transform on a qubit register (qsv_apply_qft): every stage whose qubit lies in an LDS-resident tile
// runs in the same pass over HBM (k_qft_tile, modelled on k_pass_tile of qsv_pass.hip); the planning arithmetic and the
// statement of the twiddle angles are qsv_qft_plan.h.  The reversal of the qubits goes through qsvk_permute.
//
// Twiddles.  Stage r multiplies by t = exp(2 pi i T / 2^L) with T = X mod 2^(L-1), X the integer the transform's qubits
// spell in the amplitude's index.  X is split three ways: the ranks outside the tile (one value per tile, computed under
// the tile's load), the tile bits a thread does not hold in registers (one value per thread and run), and the three other
// register bits of the run (eight settings per stage).  t is the product of two factors, each one sincospi of an exactly
// reduced dyadic argument: the thread's (once per stage and thread) and the register setting's (a table of 8 per stage
// in LDS, filled once per tile under the load).  Nothing is carried from one amplitude to the next.

#include "qsv_device.h"
#include "qsv_qft_plan.h"

#include <cstdio>
#include <cstring>

namespace {

using qsv_qft_plan::Pass;
using qsv_qft_plan::qft_turns_in;
using qsv_qft_plan::qft_turns_mask;
using qsv_qft_plan::qft_turns_out;
using qsv_qft_plan::RUN_BITS;
using qsv_qft_plan::TILE_BITS;

constexpr int QFT_THREADS = 256;
constexpr int QFT_TILE = 1 << TILE_BITS;
constexpr int QFT_ROWS_PER_WAVE = (QFT_TILE / 64) / (QFT_THREADS / 64);
constexpr int QFT_TABLE = 1 << (RUN_BITS - 1);   // settings of a run's other register bits

// exp(2 pi i turns / 2^L), conjugated on request; turns < 2^(L-1), so the argument of sincospi is a dyadic number in [0, 1)
__device__ __forceinline__ cplx qft_root(uint64_t turns, int L, bool conj) {
    double s, c;
    sincospi(ldexp(static_cast<double>(turns), 1 - L), &s, &c);
    return cplx{c, conj ? -s : s};
}

__device__ __forceinline__ amp_t qft_add(amp_t a, amp_t b) { return amp_t{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ amp_t qft_sub(amp_t a, amp_t b) { return amp_t{a.x - b.x, a.y - b.y}; }

__device__ __forceinline__ void qft_butterfly(amp_t &lo, amp_t &hi, cplx t, bool twiddle_first) {
    if (twiddle_first) hi = cmul(t, hi);
    const amp_t sum = qft_add(lo, hi), diff = qft_sub(lo, hi);
    lo = sum;
    hi = twiddle_first ? diff : cmul(t, diff);
}

// One stage on register bit K of a thread's 16 amplitudes.  w: the thread's factor; tab[j]: the factor of setting j of the
// other three register bits (bit i of j = the i-th of them, ascending).
template <int K>
__device__ __forceinline__ void qft_stage16(amp_t (&x)[16], cplx w, const amp_t *tab, bool twiddle_first) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c & (1 << K)) continue;
        const int j = ((c >> (K + 1)) << K) | (c & ((1 << K) - 1));
        const amp_t f = tab[j];      // the same address in every lane
        const cplx t = {w.re * f.x - w.im * f.y, w.re * f.y + w.im * f.x};
        qft_butterfly(x[c], x[c | (1 << K)], t, twiddle_first);
    }
}

template <bool NT>
__global__ __launch_bounds__(QFT_THREADS) void k_qft_tile(amp_t *__restrict__ a, const Pass p, uint64_t w0, uint32_t regions) {
    __shared__ amp_t tile[QFT_TILE];     // [row][64 lanes]: LDS index = tile index (bits 0..5 lane, 6..11 row)
    __shared__ amp_t table[TILE_BITS * QFT_TABLE];
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RPW = QFT_ROWS_PER_WAVE;
    const uint64_t tile_id = (regions > 1 && gridDim.x % regions == 0) ? (blockIdx.x % regions) * (gridDim.x / regions) + blockIdx.x / regions
                                                                       : blockIdx.x;
    uint64_t base = w0 + tile_id;
#pragma unroll
    for (int j = 0; j < TILE_BITS; ++j) base = insert_zero(base, static_cast<int>(p.pos[j]));
    static_assert(RPW == 16 && QFT_TILE / 64 == 64, "four row bits from i, two from the wave number");
    uint64_t row0 = base + (static_cast<uint64_t>(q & 1) << p.pos[10]) + (static_cast<uint64_t>(q >> 1) << p.pos[11]);
    auto row = [&](int i) {
        uint64_t r = row0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((i >> j) & 1) r += 1ull << p.pos[6 + j];
        return r;
    };
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll
    for (int i = 0; i < RPW; ++i) __builtin_amdgcn_global_load_lds(a + row(i) + lane, tile + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    // under the load: the tile's share of X, and the stages' tables
    const uint64_t x_out = qft_turns_out(base, p);
    const bool conj = p.conj_twiddle != 0, twiddle_first = p.twiddle_first != 0;
    if (static_cast<int>(threadIdx.x) < p.n_stages * QFT_TABLE) {
        const int s = threadIdx.x / QFT_TABLE, j = threadIdx.x % QFT_TABLE;
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < RUN_BITS - 1; ++k) {
            const int shift = p.reg_shift[s][k];
            if (((j >> k) & 1) && shift >= 0) x |= 1ull << shift;
        }
        const int L = p.L[s];
        const cplx w = qft_root(x & qft_turns_mask(L), L, conj);
        table[threadIdx.x] = amp_t{w.re, w.im};
    }
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < p.n_runs; ++u) {
        const int q0 = p.run_q[u][0], q1 = p.run_q[u][1], q2 = p.run_q[u][2], q3 = p.run_q[u][3];
        // this thread's setting of the other eight tile bits: its index with zeros inserted at the register bits
        uint32_t g0 = threadIdx.x;
        g0 = static_cast<uint32_t>(insert_zero(g0, q0));
        g0 = static_cast<uint32_t>(insert_zero(g0, q1));
        g0 = static_cast<uint32_t>(insert_zero(g0, q2));
        g0 = static_cast<uint32_t>(insert_zero(g0, q3));
        amp_t x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c)
            x[c] = tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)];
        const uint64_t x_thread = x_out | qft_turns_in(g0, p);   // the register bits read as zero here: they are the table's
#pragma unroll 1
        for (int s = p.run_first[u]; s < p.run_first[u] + p.run_count[u]; ++s) {
            const int L = p.L[s];
            const cplx w = qft_root(x_thread & qft_turns_mask(L), L, conj);
            const amp_t *tab = table + s * QFT_TABLE;
            switch (p.reg[s]) {           // wave-uniform
                case 0: qft_stage16<0>(x, w, tab, twiddle_first); break;
                case 1: qft_stage16<1>(x, w, tab, twiddle_first); break;
                case 2: qft_stage16<2>(x, w, tab, twiddle_first); break;
                default: qft_stage16<3>(x, w, tab, twiddle_first); break;
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c)
            tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)] = x[c];
        __syncthreads();
    }
    const double scale = p.scale;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const amp_t v = tile[(q * RPW + i) * 64 + lane];
        st<NT>(a + row(i) + lane, amp_t{v.x * scale, v.y * scale});
    }
}

// Registers below 2^12 amplitudes: one workgroup, the whole register in LDS, one stage after the other on the pairs.
__global__ __launch_bounds__(QFT_THREADS) void k_qft_small(amp_t *__restrict__ a, const Pass p) {
    __shared__ amp_t tile[QFT_TILE / 2];
    const uint32_t amps = 1u << p.tile_bits;
    for (uint32_t i = threadIdx.x; i < amps; i += QFT_THREADS) tile[i] = a[i];
    __syncthreads();
    const bool conj = p.conj_twiddle != 0, twiddle_first = p.twiddle_first != 0;
    for (int s = 0; s < p.n_stages; ++s) {
        const int k = p.tile_index[s], L = p.L[s];
        for (uint32_t w = threadIdx.x; w < amps / 2; w += QFT_THREADS) {
            const uint32_t i0 = static_cast<uint32_t>(insert_zero(w, k)), i1 = i0 | (1u << k);
            const cplx t = qft_root(qft_turns_in(i0, p) & qft_turns_mask(L), L, conj);
            amp_t lo = tile[i0], hi = tile[i1];
            qft_butterfly(lo, hi, t, twiddle_first);
            tile[i0] = lo;
            tile[i1] = hi;
        }
        __syncthreads();
    }
    const double scale = p.scale;
    for (uint32_t i = threadIdx.x; i < amps; i += QFT_THREADS) a[i] = amp_t{tile[i].x * scale, tile[i].y * scale};
}

int launch_pass(qsv_state *st, const Pass &p) {
    if (p.tile_bits < TILE_BITS) {
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_qft_small");
        hipLaunchKernelGGL(k_qft_small, dim3(1), dim3(QFT_THREADS), 0, st->stream, st->data, p);
        return check_launch();
    }
    const bool nt = st->nontemporal != 0;
    const uint32_t regions = st->remap >= 0 ? static_cast<uint32_t>(st->remap) : 8u;
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_qft_tile<%s>", nt ? "true" : "false");
    for (const qsv_layout::Range &r : qsv_layout::dispatch_ranges(st->amps >> TILE_BITS, qsv_layout::DISPATCH_TILES)) {
        const dim3 gd(static_cast<unsigned>(r.count)), bd(QFT_THREADS);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_qft_tile<NT.value>, gd, bd, 0, st->stream, st->data, p, r.w0, regions); });
        const int rc = check_launch();
        if (rc) return rc;
    }
    return QSV_OK;
}

}  // namespace

// bits[r] = index bit of the transform's qubit r.  *launches counts the tile passes and the permutation.
int qsvk_qft(qsv_state *st, int m, const int *bits, int flags, uint64_t *launches) {
    const std::vector<int> b(bits, bits + m);
    const std::vector<Pass> plan = qsv_qft_plan::qft_plan(st->n, b, flags);
    int src_bit_of_dst_bit[qsv_qft_plan::MAX_QUBITS];
    const bool swaps = !(flags & qsv_qft_plan::NO_SWAPS) && qsv_qft_plan::qft_reversal(st->n, b, src_bit_of_dst_bit);
    const bool inverse = (flags & qsv_qft_plan::INVERSE) != 0;
    *launches = 0;
    if (swaps && inverse) {
        const int rc = qsvk_permute(st, src_bit_of_dst_bit);
        if (rc) return rc;
        ++*launches;
    }
    for (const Pass &p : plan) {
        const int rc = launch_pass(st, p);
        if (rc) return rc;
        ++*launches;
    }
    if (swaps && !inverse) {
        const int rc = qsvk_permute(st, src_bit_of_dst_bit);
        if (rc) return rc;
        ++*launches;
    }
    return QSV_OK;
}

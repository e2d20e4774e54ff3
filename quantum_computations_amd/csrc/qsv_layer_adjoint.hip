// The adjoint walk through a product layer (gfx950, wave64): qsv_layer_adjoint and qsv_layer_transition.
// For every stage of qsv_apply_layer's plan (qsv_layer_plan.h, unchanged) the 2x2 transition matrix
//     T[a][b] = sum over the other index bits of conj(lambda[a, rest]) psi[b, rest]
// is formed from the LDS tile in which the stage is then applied to BOTH registers with qsv_layer_item.h's one statement,
// so the registers come out bit for bit as qsv_apply_layer leaves them, in the forward plan's max(1, ceil(h / 6)) launches.
//   k_layer_adjoint_tile<NT, APPLY>   k_layer_tile's skeleton on two registers: the tile's rows of psi and of lambda go straight
//                                     from HBM into two 64 KiB LDS tiles (one workgroup per CU), runs of four stages in
//                                     registers (16 amplitudes of each register per thread), one LDS round trip per run, one
//                                     store per register.  A workgroup walks tiles blockIdx.x, + gridDim.x, ... on a capped
//                                     grid and keeps its sums across them.  The matrices are kernel arguments.
//   k_layer_adjoint_small<NT, APPLY>  registers below 2^12 amplitudes, k_layer_small's shape: both registers in LDS (one
//                                     chunk, so one workgroup), one stage after the other on the pairs, a barrier between.
// APPLY = false (qsv_layer_transition) skips the stage's arithmetic, the LDS write-back and the stores.
// THE SUMS.  A stage's eight doubles: per thread over its pairs in index order; over the wave by a butterfly of shuffles
// (xor 32, 16, ... 1); the wave's first lane adds them to the wave's own LDS slot of the stage, tile after tile; at the end the
// four slots are added in wave order into partials[workgroup][stage][8]; the host adds the workgroups in index order.  No
// atomics: the same grid gives the same bits.  Scratch: grid x k x 8 doubles for the whole call, grid <= QSV_REDUCE_BLOCKS
// (1024; QSV_OPT_GRID_CAP lowers it) -- at most 64 KiB per stage, 1.75 MiB for a full wall on 28 qubits.

#include "qsv_ensemble_device.h"
#include "qsv_layer_item.h"
#include "qsv_layer_plan.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace {

using qsv_layer_plan::MATRIX_DOUBLES;
using qsv_layer_plan::Pass;
using qsv_layer_plan::TILE_BITS;

constexpr int ADJ_THREADS = 256;
constexpr int ADJ_WAVES = ADJ_THREADS / 64;
constexpr int ADJ_TILE = 1 << TILE_BITS;
constexpr int ADJ_ROWS_PER_WAVE = (ADJ_TILE / 64) / ADJ_WAVES;
constexpr int ADJ_SMALL = 1 << (TILE_BITS - 1);       // k_layer_adjoint_small: at most 2^11 amplitudes of each register
constexpr int VALUE_DOUBLES = 8;                      // one 2x2 complex transition matrix

// the matrices of one pass: kernel arguments (scalar loads)
struct PassMatrices {
    double m[TILE_BITS][MATRIX_DOUBLES];
};

// t[a][b] += conj(l_a) p_b for the pair (a = 0 / 1: the stage's index bit), with the fused multiply-adds spelled out so that
// both kernel forms round alike
__device__ __forceinline__ void adjoint_products(amp_t la, amp_t lb, amp_t pa, amp_t pb, double (&t)[VALUE_DOUBLES]) {
    t[0] = fma(la.x, pa.x, fma(la.y, pa.y, t[0]));
    t[1] = fma(la.x, pa.y, fma(-la.y, pa.x, t[1]));
    t[2] = fma(la.x, pb.x, fma(la.y, pb.y, t[2]));
    t[3] = fma(la.x, pb.y, fma(-la.y, pb.x, t[3]));
    t[4] = fma(lb.x, pa.x, fma(lb.y, pa.y, t[4]));
    t[5] = fma(lb.x, pa.y, fma(-lb.y, pa.x, t[5]));
    t[6] = fma(lb.x, pb.x, fma(lb.y, pb.y, t[6]));
    t[7] = fma(lb.x, pb.y, fma(-lb.y, pb.x, t[7]));
}

// the butterfly over the wave: every lane ends with the wave's sums
__device__ __forceinline__ void adjoint_wave_sums(double (&t)[VALUE_DOUBLES]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int e = 0; e < VALUE_DOUBLES; ++e) t[e] += __shfl_xor(t[e], o, 64);
    }
}

// One stage on register bit K of a thread's 16 amplitudes of each register: the products of its 8 pairs, then the stage.
template <int K, bool APPLY>
__device__ __forceinline__ void adjoint_stage16(amp_t (&x)[16], amp_t (&l)[16], const LayerMatrix &m, double (&t)[VALUE_DOUBLES]) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c & (1 << K)) continue;
        adjoint_products(l[c], l[c | (1 << K)], x[c], x[c | (1 << K)], t);
        if constexpr (APPLY) {
            layer_item(x[c], x[c | (1 << K)], m);
            layer_item(l[c], l[c | (1 << K)], m);
        }
    }
}

// partials[(blockIdx.x * p.n_stages + s) * 8 + e]: the workgroup's share of stage s of this pass.  tiles = amps >> 12.
template <bool NT, bool APPLY>
__global__ __launch_bounds__(ADJ_THREADS) void k_layer_adjoint_tile(amp_t *__restrict__ psi, amp_t *__restrict__ lambda, const Pass p,
                                                                    const PassMatrices shared, uint64_t tiles, double *__restrict__ partials) {
    __shared__ amp_t tile_p[ADJ_TILE];     // [row][64 lanes]: LDS index = tile index (bits 0..5 lane, 6..11 row)
    __shared__ amp_t tile_l[ADJ_TILE];
    __shared__ double sums[TILE_BITS][ADJ_WAVES][VALUE_DOUBLES];     // a wave's slot is written by its first lane only
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RPW = ADJ_ROWS_PER_WAVE;
    static_assert(RPW == 16 && ADJ_TILE / 64 == 64, "four row bits from i, two from the wave number");
    for (int i = threadIdx.x; i < TILE_BITS * ADJ_WAVES * VALUE_DOUBLES; i += ADJ_THREADS) (&sums[0][0][0])[i] = 0.0;
    for (uint64_t tile_id = blockIdx.x; tile_id < tiles; tile_id += gridDim.x) {
        uint64_t base = tile_id;
#pragma unroll
        for (int j = 0; j < TILE_BITS; ++j) base = insert_zero(base, static_cast<int>(p.pos[j]));
        const uint64_t row0 = base + (static_cast<uint64_t>(q & 1) << p.pos[10]) + (static_cast<uint64_t>(q >> 1) << p.pos[11]);
        auto row = [&](int i) {
            uint64_t r = row0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((i >> j) & 1) r += 1ull << p.pos[6 + j];
            return r;
        };
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll 4
        for (int i = 0; i < RPW; ++i) {
            __builtin_amdgcn_global_load_lds(psi + row(i) + lane, tile_p + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
            __builtin_amdgcn_global_load_lds(lambda + row(i) + lane, tile_l + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
        }
#endif
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
            amp_t x[16], l[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const uint32_t at = g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3);
                x[c] = tile_p[at];
                l[c] = tile_l[at];
            }
#pragma unroll 1
            for (int s = p.run_first[u]; s < p.run_first[u] + p.run_count[u]; ++s) {
                const LayerMatrix m = layer_matrix(shared.m[s]);
                double t[VALUE_DOUBLES];
#pragma unroll
                for (int e = 0; e < VALUE_DOUBLES; ++e) t[e] = 0.0;
                switch (p.reg[s]) {           // wave-uniform
                    case 0: adjoint_stage16<0, APPLY>(x, l, m, t); break;
                    case 1: adjoint_stage16<1, APPLY>(x, l, m, t); break;
                    case 2: adjoint_stage16<2, APPLY>(x, l, m, t); break;
                    default: adjoint_stage16<3, APPLY>(x, l, m, t); break;
                }
                adjoint_wave_sums(t);
                if (lane == 0) {
#pragma unroll
                    for (int e = 0; e < VALUE_DOUBLES; ++e) sums[s][q][e] += t[e];
                }
            }
            if constexpr (APPLY) {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint32_t at = g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3);
                    tile_p[at] = x[c];
                    tile_l[at] = l[c];
                }
                __syncthreads();
            }
        }
        if constexpr (APPLY) {
#pragma unroll 4
            for (int i = 0; i < RPW; ++i) {
                st<NT>(psi + row(i) + lane, tile_p[(q * RPW + i) * 64 + lane]);
                st<NT>(lambda + row(i) + lane, tile_l[(q * RPW + i) * 64 + lane]);
            }
        }
        __syncthreads();     // the next tile fills both LDS tiles again
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < p.n_stages * VALUE_DOUBLES) {
        const int s = threadIdx.x / VALUE_DOUBLES, e = threadIdx.x % VALUE_DOUBLES;
        double sum = 0.0;
        for (int w = 0; w < ADJ_WAVES; ++w) sum += sums[s][w][e];
        partials[(static_cast<uint64_t>(blockIdx.x) * p.n_stages + s) * VALUE_DOUBLES + e] = sum;
    }
}

// Below one tile: n <= 11 bits, both registers whole in LDS, one workgroup.  partials[s * 8 + e].
template <bool NT, bool APPLY>
__global__ __launch_bounds__(ADJ_THREADS) void k_layer_adjoint_small(amp_t *__restrict__ psi, amp_t *__restrict__ lambda, const Pass p,
                                                                     const PassMatrices shared, int n, double *__restrict__ partials) {
    __shared__ amp_t tile_p[ADJ_SMALL];
    __shared__ amp_t tile_l[ADJ_SMALL];
    __shared__ double sums[ADJ_WAVES][VALUE_DOUBLES];
    const uint32_t amps = 1u << n, pairs = amps >> 1;
    for (uint32_t i = threadIdx.x; i < amps; i += ADJ_THREADS) {
        tile_p[i] = ld<NT>(psi + i);
        tile_l[i] = ld<NT>(lambda + i);
    }
    __syncthreads();
    for (int s = 0; s < p.n_stages; ++s) {
        const int bit = p.bit[s];
        const LayerMatrix m = layer_matrix(shared.m[s]);
        double t[VALUE_DOUBLES];
#pragma unroll
        for (int e = 0; e < VALUE_DOUBLES; ++e) t[e] = 0.0;
        for (uint32_t w = threadIdx.x; w < pairs; w += ADJ_THREADS) {
            const uint32_t i0 = static_cast<uint32_t>(qsv_layer_plan::pair_low(w, bit)), i1 = i0 | (1u << bit);
            amp_t pa = tile_p[i0], pb = tile_p[i1], la = tile_l[i0], lb = tile_l[i1];
            adjoint_products(la, lb, pa, pb, t);
            if constexpr (APPLY) {
                layer_item(pa, pb, m);
                layer_item(la, lb, m);
                tile_p[i0] = pa;
                tile_p[i1] = pb;
                tile_l[i0] = la;
                tile_l[i1] = lb;
            }
        }
        adjoint_wave_sums(t);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int e = 0; e < VALUE_DOUBLES; ++e) sums[threadIdx.x >> 6][e] = t[e];
        }
        __syncthreads();     // the stage's pairs are written and its sums are in LDS
        if (threadIdx.x < VALUE_DOUBLES) {
            double sum = 0.0;
            for (int w = 0; w < ADJ_WAVES; ++w) sum += sums[w][threadIdx.x];
            partials[s * VALUE_DOUBLES + threadIdx.x] = sum;
        }
        __syncthreads();     // the next stage writes the sums again
    }
    if constexpr (APPLY) {
        for (uint32_t i = threadIdx.x; i < amps; i += ADJ_THREADS) {
            st<NT>(psi + i, tile_p[i]);
            st<NT>(lambda + i, tile_l[i]);
        }
    }
}

const char *tf(bool v) { return v ? "true" : "false"; }

// workgroups of a pass: one for the small form, else one per tile up to the cap of the reductions (QSV_OPT_GRID_CAP lowers it)
int adjoint_grid(const qsv_state *st, const Pass &p) {
    if (p.tile_bits < TILE_BITS) return 1;
    const int cap = st->grid_cap > 0 && st->grid_cap < QSV_REDUCE_BLOCKS ? st->grid_cap : QSV_REDUCE_BLOCKS;
    return grid_for(st->amps >> TILE_BITS, 1, cap);
}

// One pass over both registers on psi's stream.  host: the layer's matrices in stage order (APPLY only).
int launch_pass(qsv_state *psi, amp_t *lambda, const Pass &p, const double *host, bool apply, int grid, double *partials) {
    const bool nt = psi->nontemporal != 0;
    PassMatrices shared = {};
    if (apply)
        for (int s = 0; s < p.n_stages; ++s)
            for (int e = 0; e < MATRIX_DOUBLES; ++e) shared.m[s][e] = host[static_cast<size_t>(p.first + s) * MATRIX_DOUBLES + e];
    const dim3 gd(static_cast<unsigned>(grid)), bd(ADJ_THREADS);
    if (p.tile_bits < TILE_BITS) {
        snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_layer_adjoint_small<%s, %s>", tf(nt), tf(apply));
        with_bool(nt, [&](auto NT) { with_bool(apply, [&](auto APPLY) {
            hipLaunchKernelGGL((k_layer_adjoint_small<NT.value, APPLY.value>), gd, bd, 0, psi->stream, psi->data, lambda, p, shared, psi->n, partials);
        }); });
        return check_launch();
    }
    snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_layer_adjoint_tile<%s, %s>", tf(nt), tf(apply));
    with_bool(nt, [&](auto NT) { with_bool(apply, [&](auto APPLY) {
        hipLaunchKernelGGL((k_layer_adjoint_tile<NT.value, APPLY.value>), gd, bd, 0, psi->stream, psi->data, lambda, p, shared,
                           psi->amps >> TILE_BITS, partials);
    }); });
    return check_launch();
}

// what both calls refuse, in check_layer's words (qsv_layer.hip); psi is the ket, lambda the bra
int check_walk(const qsv_state *psi, const qsv_state *lambda, int k, const int *qubits, const double *inverse, const double *values, bool apply) {
    if (!psi || !lambda) return qsv_fail(QSV_EINVAL, "null pointer");
    if (psi->kind != 0 || lambda->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    if (psi->n != lambda->n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    if (psi->device != lambda->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    const int n = psi->n;
    if (k < 0 || k > n) return qsv_fail(QSV_EINVAL, "a layer takes between 0 and " + std::to_string(n) + " qubits, not " + std::to_string(k));
    if (k > 0 && (!qubits || !values || (apply && !inverse))) return qsv_fail(QSV_EINVAL, "null pointer");
    const int rc = check_member_qubits(n, k, qubits);      // the qubit-list refusals of qsv_apply_layer, in the same words
    if (rc) return rc;
    if (apply) {
        for (size_t i = 0; i < static_cast<size_t>(k) * MATRIX_DOUBLES; ++i)
            if (!std::isfinite(inverse[i])) return qsv_fail(QSV_EINVAL, "every matrix entry must be finite");
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(psi->data), b0 = reinterpret_cast<uintptr_t>(lambda->data);
        if (psi == lambda || (a0 < b0 + sizeof(amp_t) * lambda->amps && b0 < a0 + sizeof(amp_t) * psi->amps))
            return qsv_fail(QSV_EINVAL, "the two registers must not share memory");
    }
    return QSV_OK;
}

int walk(qsv_state *psi, qsv_state *lambda, int k, const int *qubits, const double *inverse, double *values, uint64_t *passes, bool apply) {
    int rc = check_walk(psi, lambda, k, qubits, inverse, values, apply);
    if (rc) return rc;
    if (passes) *passes = 0;
    if (k == 0) return QSV_OK;
    rc = qsv_flush(psi);
    if (rc) return rc;
    if (lambda != psi) {
        rc = qsv_flush(lambda);
        if (rc) return rc;
    }
    QSV_HIP(hipSetDevice(psi->device));
    if (lambda != psi) QSV_HIP(hipStreamSynchronize(lambda->stream));
    const int n = psi->n;
    std::vector<int> bits(k);
    for (int i = 0; i < k; ++i) bits[i] = n - 1 - qubits[i];
    const qsv_layer_plan::Layer plan = qsv_layer_plan::layer_plan(n, bits);
    std::vector<double> host_m;
    if (apply) {
        host_m.resize(static_cast<size_t>(k) * MATRIX_DOUBLES);
        for (int s = 0; s < k; ++s)
            for (int e = 0; e < MATRIX_DOUBLES; ++e) host_m[static_cast<size_t>(s) * MATRIX_DOUBLES + e] = inverse[static_cast<size_t>(plan.order[s]) * MATRIX_DOUBLES + e];
    }
    // every pass has its own slice of psi's scratch buffer: grid x stages x 8 doubles
    std::vector<size_t> offset;
    std::vector<int> grids;
    size_t doubles = 0;
    for (const Pass &p : plan.passes) {
        const int grid = adjoint_grid(psi, p);
        offset.push_back(doubles);
        grids.push_back(grid);
        doubles += static_cast<size_t>(grid) * p.n_stages * VALUE_DOUBLES;
    }
    rc = qsvk_ensure_matrix(psi, sizeof(double) * doubles);
    if (rc) return rc;
    for (size_t i = 0; i < plan.passes.size(); ++i) {
        rc = launch_pass(psi, lambda->data, plan.passes[i], host_m.data(), apply, grids[i], psi->dev_matrix + offset[i]);
        if (rc) {
            (void)hipStreamSynchronize(psi->stream);
            return rc;
        }
    }
    std::vector<double> host(doubles);
    QSV_HIP(hipMemcpyAsync(host.data(), psi->dev_matrix, sizeof(double) * doubles, hipMemcpyDeviceToHost, psi->stream));
    QSV_HIP(hipStreamSynchronize(psi->stream));
    for (size_t i = 0; i < plan.passes.size(); ++i) {
        const Pass &p = plan.passes[i];
        for (int s = 0; s < p.n_stages; ++s)
            for (int e = 0; e < VALUE_DOUBLES; ++e) {
                double sum = 0.0;
                for (int b = 0; b < grids[i]; ++b) sum += host[offset[i] + (static_cast<size_t>(b) * p.n_stages + s) * VALUE_DOUBLES + e];
                values[static_cast<size_t>(plan.order[p.first + s]) * VALUE_DOUBLES + e] = sum;
            }
    }
    if (passes) *passes = plan.passes.size();
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_layer_adjoint(qsv_state *psi, qsv_state *lambda, int k, const int *qubits, const double *inverse, double *values, uint64_t *passes) {
    return walk(psi, lambda, k, qubits, inverse, values, passes, true);
}

int qsv_layer_transition(qsv_state *bra, qsv_state *ket, int k, const int *qubits, double *values, uint64_t *passes) {
    return walk(ket, bra, k, qubits, nullptr, values, passes, false);
}

}  // extern "C"

// Product layers (gfx950, wave64): a 2x2 matrix on each of k distinct qubits of a register (qsv_apply_layer) or of every
// member of an ensemble, each member with matrices of its own (qsv_ensemble_apply_layer), in max(1, ceil(h / 6)) passes over
// HBM, h = the stage bits >= 6, instead of k.  The plan is qsv_layer_plan.h, the arithmetic of a
// stage qsv_layer_item.h: one statement for every form, so a member rounds exactly as a register of its own does.
//   k_layer_tile<NT, PER_MEMBER>   one workgroup per 4096-amplitude tile, k_qft_tile's skeleton (qsv_qft.hip): rows straight
//                                  from HBM into LDS, runs of four stages in registers, one LDS round trip per run, one store.
//                                  Shared matrices come from the kernel arguments (scalar loads); a member's matrices are
//                                  requested before the tile's rows and parked in LDS while the rows are in flight.
//   k_layer_small<NT, PER_MEMBER>  registers and members below 2^12 amplitudes: a workgroup walks chunks of 2^min(11, total
//                                  bits) amplitudes -- whole members -- in LDS, one stage after the other on the pairs; a
//                                  pair never leaves its member and takes the matrix of the member it lies in.
// In place, no scratch, one launch per pass (dispatch_ranges splits a grid beyond 2^23 tiles).

#include "qsv_ensemble_device.h"
#include "qsv_layer_item.h"
#include "qsv_layer_plan.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace {

using qsv_layer_plan::MATRIX_DOUBLES;
using qsv_layer_plan::Pass;
using qsv_layer_plan::RUN_BITS;
using qsv_layer_plan::TILE_BITS;

constexpr int LAYER_THREADS = 256;
constexpr int LAYER_TILE = 1 << TILE_BITS;
constexpr int LAYER_ROWS_PER_WAVE = (LAYER_TILE / 64) / (LAYER_THREADS / 64);
constexpr int LAYER_SMALL_BITS = TILE_BITS - 1;       // chunk of k_layer_small: at most 2^11 amplitudes
constexpr int LAYER_SMALL = 1 << LAYER_SMALL_BITS;

// the matrices of one pass where every member takes the same: kernel arguments
struct PassMatrices {
    double m[TILE_BITS][MATRIX_DOUBLES];
};

// One stage on register bit K of a thread's 16 amplitudes.
template <int K>
__device__ __forceinline__ void layer_stage16(amp_t (&x)[16], const LayerMatrix &m) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c & (1 << K)) continue;
        layer_item(x[c], x[c | (1 << K)], m);
    }
}

// n: bits of a member (PER_MEMBER only); k: stages of the whole layer, the length of a member's row of `table`.
template <bool NT, bool PER_MEMBER>
__global__ __launch_bounds__(LAYER_THREADS) void k_layer_tile(amp_t *__restrict__ a, const Pass p, const PassMatrices shared, const double *__restrict__ table,
                                                              int n, int k, uint64_t w0, uint32_t regions) {
    __shared__ amp_t tile[LAYER_TILE];     // [row][64 lanes]: LDS index = tile index (bits 0..5 lane, 6..11 row)
    __shared__ double member_m[TILE_BITS * MATRIX_DOUBLES];
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RPW = LAYER_ROWS_PER_WAVE;
    const uint64_t tile_id = (regions > 1 && gridDim.x % regions == 0) ? (blockIdx.x % regions) * (gridDim.x / regions) + blockIdx.x / regions
                                                                       : blockIdx.x;
    uint64_t base = w0 + tile_id;
#pragma unroll
    for (int j = 0; j < TILE_BITS; ++j) base = insert_zero(base, static_cast<int>(p.pos[j]));
    // the member's matrices of this pass: requested first, written to LDS once the rows have been requested too
    double mine = 0.0;
    const bool fetch = PER_MEMBER && static_cast<int>(threadIdx.x) < p.n_stages * MATRIX_DOUBLES;
    if (fetch) mine = table[qsv_layer_plan::table_offset(base >> n, k, p.first) + threadIdx.x];
    static_assert(RPW == 16 && LAYER_TILE / 64 == 64, "four row bits from i, two from the wave number");
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
    if (fetch) member_m[threadIdx.x] = mine;
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
#pragma unroll 1
        for (int s = p.run_first[u]; s < p.run_first[u] + p.run_count[u]; ++s) {
            // one address per wave either way: scalar loads of the kernel arguments, or an LDS broadcast
            LayerMatrix m;
            if constexpr (PER_MEMBER)
                m = layer_matrix(member_m + s * MATRIX_DOUBLES);
            else
                m = layer_matrix(shared.m[s]);
            switch (p.reg[s]) {           // wave-uniform
                case 0: layer_stage16<0>(x, m); break;
                case 1: layer_stage16<1>(x, m); break;
                case 2: layer_stage16<2>(x, m); break;
                default: layer_stage16<3>(x, m); break;
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c)
            tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)] = x[c];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) st<NT>(a + row(i) + lane, tile[(q * RPW + i) * 64 + lane]);
}

// Below one tile.  chunk_bits = min(11, bits of the whole register) >= n: a chunk is 2^(chunk_bits - n) whole members.  A
// workgroup walks chunks; the pass's stages run one after the other on the chunk's pairs, a barrier between them.
template <bool NT, bool PER_MEMBER>
__global__ __launch_bounds__(LAYER_THREADS) void k_layer_small(amp_t *__restrict__ a, const Pass p, const PassMatrices shared, const double *__restrict__ table,
                                                               int n, int k, int chunk_bits, uint64_t chunks) {
    __shared__ amp_t tile[LAYER_SMALL];
    const uint32_t amps = 1u << chunk_bits, pairs = amps >> 1;
    for (uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        amp_t *ac = a + (chunk << chunk_bits);
        const uint64_t member0 = chunk << (chunk_bits - n);
        for (uint32_t i = threadIdx.x; i < amps; i += LAYER_THREADS) tile[i] = ld<NT>(ac + i);
        __syncthreads();
        for (int s = 0; s < p.n_stages; ++s) {
            const int bit = p.bit[s];
            for (uint32_t w = threadIdx.x; w < pairs; w += LAYER_THREADS) {
                const uint32_t i0 = static_cast<uint32_t>(qsv_layer_plan::pair_low(w, bit)), i1 = i0 | (1u << bit);
                LayerMatrix m;
                if constexpr (PER_MEMBER)
                    m = layer_matrix(table + qsv_layer_plan::table_offset(member0 + (i0 >> n), k, p.first + s));
                else
                    m = layer_matrix(shared.m[s]);
                amp_t lo = tile[i0], hi = tile[i1];
                layer_item(lo, hi, m);
                tile[i0] = lo;
                tile[i1] = hi;
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < amps; i += LAYER_THREADS) st<NT>(ac + i, tile[i]);
        __syncthreads();     // the next chunk fills the tile again
    }
}

const char *tf(bool v) { return v ? "true" : "false"; }

// One pass on the whole register.  n: bits of a member (of the register where table == nullptr); host: the layer's
// matrices in stage order (shared form only).
int launch_pass(qsv_state *st, const Pass &p, int n, int k, const double *host, const double *table) {
    const bool per_member = table != nullptr, nt = st->nontemporal != 0;
    PassMatrices shared = {};
    if (!per_member)
        for (int s = 0; s < p.n_stages; ++s)
            for (int e = 0; e < MATRIX_DOUBLES; ++e) shared.m[s][e] = host[static_cast<size_t>(p.first + s) * MATRIX_DOUBLES + e];
    if (p.tile_bits < TILE_BITS) {
        const int chunk_bits = std::min(LAYER_SMALL_BITS, st->n);
        const uint64_t chunks = st->amps >> chunk_bits;
        const dim3 gd(static_cast<unsigned>(grid_for(chunks, 1, st->grid_cap))), bd(LAYER_THREADS);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_layer_small<%s, %s>", tf(nt), tf(per_member));
        with_bool(nt, [&](auto NT) { with_bool(per_member, [&](auto PM) {
            hipLaunchKernelGGL((k_layer_small<NT.value, PM.value>), gd, bd, 0, st->stream, st->data, p, shared, table, n, k, chunk_bits, chunks);
        }); });
        return check_launch();
    }
    const uint32_t regions = regions_or(st, 8u);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_layer_tile<%s, %s>", tf(nt), tf(per_member));
    for (const qsv_layout::Range &r : qsv_layout::dispatch_ranges(st->amps >> TILE_BITS, qsv_layout::DISPATCH_TILES)) {
        const dim3 gd(static_cast<unsigned>(r.count)), bd(LAYER_THREADS);
        with_bool(nt, [&](auto NT) { with_bool(per_member, [&](auto PM) {
            hipLaunchKernelGGL((k_layer_tile<NT.value, PM.value>), gd, bd, 0, st->stream, st->data, p, shared, table, n, k, r.w0, regions);
        }); });
        const int rc = check_launch();
        if (rc) return rc;
    }
    return QSV_OK;
}

// what both calls refuse about the list and the matrices; n = qubits of the register or of a member
int check_layer(int n, int k, const int *qubits, const double *matrices, uint64_t members) {
    if (k < 0 || k > n) return qsv_fail(QSV_EINVAL, "a layer takes between 0 and " + std::to_string(n) + " qubits, not " + std::to_string(k));
    if (k > 0 && (!qubits || !matrices)) return qsv_fail(QSV_EINVAL, "null pointer");
    const int rc = check_member_qubits(n, k, qubits);
    if (rc) return rc;
    const size_t count = static_cast<size_t>(members) * k * MATRIX_DOUBLES;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(matrices[i])) return qsv_fail(QSV_EINVAL, "every matrix entry must be finite");
    return QSV_OK;
}

std::vector<int> bits_of(int n, int k, const int *qubits) {
    std::vector<int> bits(k);
    for (int i = 0; i < k; ++i) bits[i] = n - 1 - qubits[i];
    return bits;
}

}  // namespace

extern "C" {

int qsv_apply_layer(qsv_state *st, int k, const int *qubits, const double *matrices, uint64_t *passes) {
    if (!st) return qsv_fail(QSV_EINVAL, "null pointer");
    if (st->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs a qubit register");
    int rc = check_layer(st->n, k, qubits, matrices, 1);
    if (rc) return rc;
    if (passes) *passes = 0;
    if (k == 0) return QSV_OK;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    const qsv_layer_plan::Layer plan = qsv_layer_plan::layer_plan(st->n, bits_of(st->n, k, qubits));
    std::vector<double> host(static_cast<size_t>(k) * MATRIX_DOUBLES);
    for (int s = 0; s < k; ++s)
        for (int e = 0; e < MATRIX_DOUBLES; ++e) host[static_cast<size_t>(s) * MATRIX_DOUBLES + e] = matrices[static_cast<size_t>(plan.order[s]) * MATRIX_DOUBLES + e];
    for (const Pass &p : plan.passes) {
        rc = launch_pass(st, p, st->n, k, host.data(), nullptr);
        if (rc) return rc;
    }
    if (passes) *passes = plan.passes.size();
    return QSV_OK;
}

int qsv_ensemble_apply_layer(qsv_state *st, int member_qubits, int k, const int *qubits, const double *matrices, uint64_t *passes) {
    int rc = check_ensemble(st, member_qubits, 0);
    if (rc) return rc;
    const int n = member_qubits;
    const uint64_t members = st->amps >> n;
    rc = check_layer(n, k, qubits, matrices, members);
    if (rc) return rc;
    if (passes) *passes = 0;
    if (k == 0) return QSV_OK;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    const qsv_layer_plan::Layer plan = qsv_layer_plan::layer_plan(n, bits_of(n, k, qubits));
    // the table in stage order, one row per member
    const size_t doubles = qsv_layer_plan::table_doubles(members, k);
    std::vector<double> host(doubles);
    for (uint64_t m = 0; m < members; ++m)
        for (int s = 0; s < k; ++s) {
            const double *src = matrices + qsv_layer_plan::table_offset(m, k, plan.order[s]);
            double *dst = host.data() + qsv_layer_plan::table_offset(m, k, s);
            for (int e = 0; e < MATRIX_DOUBLES; ++e) dst[e] = src[e];
        }
    rc = qsvk_ensure_matrix(st, sizeof(double) * doubles);
    if (rc) return rc;
    // pageable memory: the copy has left `host` when this returns, and is ordered on the register's stream
    QSV_HIP(hipMemcpyAsync(st->dev_matrix, host.data(), sizeof(double) * doubles, hipMemcpyHostToDevice, st->stream));
    for (const Pass &p : plan.passes) {
        rc = launch_pass(st, p, n, k, nullptr, st->dev_matrix);
        if (rc) return rc;
    }
    if (passes) *passes = plan.passes.size();
    return QSV_OK;
}

}  // extern "C"

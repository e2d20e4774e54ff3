// Subsystem read-out of the qubit register (gfx950, wave64): the reduced state of up to 12 qubits,
// left on the device as a density register, and the marginal distribution of up to 26, with their C entry points.
//
//   k_subsys_tile      rho_A = M M^dagger on the f64 matrix cores.  The 2^k rows are cut into blocks of 64, only block
//                      pairs I <= J are computed, and the traced index is cut into slices: a work item is (block pair,
//                      slice).  It stages 64 rows of I and 64 rows of J for 32 groups at a time through a swizzled LDS
//                      tile (the wave-load scheme of k_rdm_tile: 64 consecutive amplitudes per load, kept bits below 6 in
//                      the lane, kept bits from 6 up in the load's address) and accumulates 16 x 16 tiles with
//                      v_mfma_f64_16x16x4 in the three-product complex form.  Wave w owns row tile w of I against the
//                      four row tiles of J: 4 pairs x 3 accumulators x 8 registers.
//   k_subsys_finish    adds the slice partials in a fixed order, writes the entries in the caller's order and mirrors
//                      the lower triangle (and traces out the positions the plan kept on top of the caller's, k < 6).
//   k_subsys_entry     registers and shapes the tiled form cannot take: one thread per entry of the upper triangle.
//   k_marginal_stream  one read pass; a wave walks its run of loads for each setting of the kept bits >= 6, lanes
//                      accumulate |x|^2, lanes that differ in traced lane bits are combined by shuffles, one partial per
//                      wave; k_sum_partials (qsv_readout.hip) adds them.
//   k_marginal_entry   one thread per output entry looping over the traced settings (large k, small registers).
// Launch shapes and index arithmetic: qsv_subsystem_layout.h.

#include "qsv_device.h"
#include "qsv_subsystem_layout.h"

#include <vector>

using namespace qsv_subsystem_layout;

static_assert(SUB_BLOCK == QSV_BLOCK && SUB_LANE_BITS == QSV_LANE_BITS && SUB_MIN_QUBITS == qsv_readout_layout::RO_MIN_QUBITS,
              "qsv_subsystem_layout.h mirrors qsv_internal.h");

namespace {

constexpr int SIDE_AMPS = SUB_ROWS * SUB_FILL_GROUPS;   // amplitudes of one block's rows in the LDS tile
constexpr int LOAD_BATCH = 8;                            // wave-loads in flight per wave before the first LDS write (8 or 16 per wave, block and fill)

__global__ __launch_bounds__(QSV_BLOCK) void k_subsys_tile(const amp_t *__restrict__ a, const SubArgs g,
                                                          double *__restrict__ partials) {   // [item][4][4][2][256]
    __shared__ __attribute__((aligned(16))) amp_t tile[2 * SIDE_AMPS];   // 64 KiB: rows of I, then rows of J
    const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    const uint32_t wave_s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t r_low, f_low;                                 // this lane's row bits and group bits in a wave-load
    sub_lane_place(g.lmask, lane, &r_low, &f_low);
    const int l = g.l;
    const uint32_t mine = sub_fill_loads(l) / 4u;          // wave-loads per wave, block and fill
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t pair = item / g.slices, slice = item % g.slices;
        uint32_t I, J;
        sub_pair_blocks(g.nb, pair, &I, &J);
        const uint32_t sides = I == J ? 1u : 2u;            // a diagonal block is staged once and read as both operands
        f64x4 p1[4], p2[4], p3[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) p1[t] = p2[t] = p3[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        const uint64_t t_first = slice * g.tiles_per_slice;
        for (uint64_t t = t_first; t < t_first + g.tiles_per_slice; ++t) {
            const uint64_t tile_bits = sub_tile_bits(g, t);
            for (uint32_t hf = 0; hf < 2; ++hf) {
                __syncthreads();                            // every wave is done with the previous fill
                for (uint32_t side = 0; side < sides; ++side) {
                    const uint64_t fill_bits = tile_bits | sub_block_bits(g, side ? J : I);   // per fill: holding both blocks' bits spills scalars
                    for (uint32_t j0 = mine * wave_s; j0 < mine * (wave_s + 1u); j0 += LOAD_BATCH) {
                        amp_t x[LOAD_BATCH];
                        uint32_t slot[LOAD_BATCH];
                        const bool active = sub_lane_active(l, f_low, hf);
#pragma unroll
                        for (int u = 0; u < LOAD_BATCH; ++u) {
                            const SubLoad ld = sub_tile_load_from(g, fill_bits, 0, hf, j0 + u);
                            slot[u] = sub_lds_slot(side, ld.row_hi | r_low, ((ld.group_hi | f_low) & 31u));
                            x[u] = active ? a[ld.base + lane] : amp_t{0.0, 0.0};   // plain loads: other block pairs read the row again
                        }
#pragma unroll
                        for (int u = 0; u < LOAD_BATCH; ++u)
                            if (active) tile[slot[u]] = x[u];
                    }
                }
                __syncthreads();
                const amp_t *ti = tile + (16 * wave_s + i) * SUB_FILL_GROUPS, *tj = tile + (sides - 1u) * SIDE_AMPS + i * SUB_FILL_GROUPS;
#pragma unroll 2
                for (int m = 0; m < SUB_FILL_GROUPS / 4; ++m) {
                    const int col = (4 * m + kk) ^ i;
                    const amp_t vi = ti[col];
                    const double vs = vi.x + vi.y;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const amp_t vj = tj[16 * tt * SUB_FILL_GROUPS + col];
                        p1[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi.x, vj.x, p1[tt], 0, 0, 0);
                        p2[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi.y, vj.y, p2[tt], 0, 0, 0);
                        p3[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs, vj.x - vj.y, p3[tt], 0, 0, 0);
                    }
                }
            }
        }
        // re = P1 + P2, im = P3 - P1 + P2 (k_rdm_tile); every wave owns its tile pairs: nothing to add across waves
        double *out = partials + static_cast<size_t>(item) * SUB_PART_DOUBLES;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double *slot_re = out + ((wave_s * 4 + tt) * 2) * 256 + r * 64 + lane;
                slot_re[0] = p1[tt][r] + p2[tt][r];
                slot_re[256] = p3[tt][r] - p1[tt][r] + p2[tt][r];
            }
    }
}

// the sum of `count` doubles `stride` apart, in a fixed tree: four interleaved chains, then (c0 + c1) + (c2 + c3)
__device__ __forceinline__ double sum_strided(const double *__restrict__ p, uint32_t count, size_t stride) {
    if (count < 4) {
        double s = 0.0;
        for (uint32_t q = 0; q < count; ++q) s += p[q * stride];
        return s;
    }
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    for (uint32_t q = 0; q < count; q += 4) {   // count is a power of two
        c0 += p[q * stride];
        c1 += p[(q + 1) * stride];
        c2 += p[(q + 2) * stride];
        c3 += p[(q + 3) * stride];
    }
    return (c0 + c1) + (c2 + c3);
}

// one thread per entry ic <= jc of the caller's matrix
__global__ __launch_bounds__(QSV_BLOCK) void k_subsys_finish(const double *__restrict__ partials, const SubArgs g,
                                                            amp_t *__restrict__ rho) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    const uint64_t D = 1ull << g.k;
    if (e >= D * D) return;
    const uint32_t ic = static_cast<uint32_t>(e >> g.k), jc = static_cast<uint32_t>(e & (D - 1));
    if (ic > jc) return;
    const uint32_t i_row = sub_caller_row(g, ic), j_row = sub_caller_row(g, jc);
    double re = 0.0, im = 0.0;
    for (uint32_t x = 0; x < (1u << g.extra); ++x) {
        const uint32_t x_row = sub_extra_row(g, x);
        uint32_t ip = i_row | x_row, jp = j_row | x_row;
        const bool mirrored = ip > jp;                   // only the upper triangle was computed: take the conjugate
        if (mirrored) {
            const uint32_t s = ip;
            ip = jp;
            jp = s;
        }
        const uint32_t pair = sub_pair_index(g.nb, ip >> SUB_ROW_BITS, jp >> SUB_ROW_BITS);
        const double *p = partials + static_cast<size_t>(pair) * g.slices * SUB_PART_DOUBLES + sub_partial_slot(ip, jp);
        const double sr = sum_strided(p, g.slices, SUB_PART_DOUBLES), si = sum_strided(p + 256, g.slices, SUB_PART_DOUBLES);
        re += sr;
        im += mirrored ? -si : si;
    }
    if (ic == jc) {
        rho[ic * D + jc] = amp_t{re, 0.0};
    } else {
        rho[ic * D + jc] = amp_t{re, im};
        rho[jc * D + ic] = amp_t{re, -im};
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_subsys_entry(const amp_t *__restrict__ a, const SubArgs g, amp_t *__restrict__ rho) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    const uint64_t D = 1ull << g.k;
    if (e >= D * D) return;
    const uint64_t ic = e >> g.k, jc = e & (D - 1);
    if (ic > jc) return;
    const uint64_t oi = sub_caller_offset(g, ic), oj = sub_caller_offset(g, jc);
    const int traced = g.n - g.k;
    double sr = 0.0, si = 0.0;
    for (uint64_t w = 0; w < g.W; ++w) {
        const uint64_t base = sub_group_offset(g, w, 0, traced);
        const amp_t x = a[base + oi], y = a[base + oj];
        sr += x.x * y.x + x.y * y.y;   // x conj(y)
        si += x.y * y.x - x.x * y.y;
    }
    if (ic == jc) {
        rho[ic * D + jc] = amp_t{sr, 0.0};
    } else {
        rho[ic * D + jc] = amp_t{sr, si};
        rho[jc * D + ic] = amp_t{sr, -si};
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_marginal_stream(const amp_t *__restrict__ a, const MargArgs g,
                                                              double *__restrict__ partials) {   // [wave][2^k], physical row order
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (QSV_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t r_low, f_low;
    sub_lane_place(g.lmask, lane, &r_low, &f_low);
    const uint32_t traced_lanes = ~g.lmask & 63u;
    const int traced = g.n - g.k;
    const uint64_t first = wave * g.run;
    for (uint32_t c_h = 0; c_h < (1u << g.h); ++c_h) {
        double acc = 0.0;
#pragma unroll 4
        for (uint64_t q = 0; q < g.run; ++q) {
            const amp_t v = __builtin_nontemporal_load(a + sub_load_base(g, first + q, c_h, g.k, traced) + lane);
            acc += v.x * v.x + v.y * v.y;
        }
        for (int b = 0; b < 6; ++b)
            if ((traced_lanes >> b) & 1u) acc += __shfl_xor(acc, 1 << b, 64);
        if ((lane & traced_lanes) == 0) partials[(static_cast<size_t>(wave) << g.k) + ((c_h << g.l) | r_low)] = acc;
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_marginal_entry(const amp_t *__restrict__ a, const MargArgs g, double *__restrict__ out) {
    const uint64_t c = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (c >= (1ull << g.k)) return;
    const uint64_t off = sub_caller_offset(g, c);
    const int traced = g.n - g.k;
    double acc = 0.0;
    for (uint64_t w = 0; w < g.W; ++w) {
        const amp_t v = a[off + sub_group_offset(g, w, 0, traced)];
        acc += v.x * v.x + v.y * v.y;
    }
    out[c] = acc;
}

// everything both calls refuse about the register and the qubit list
int check_subsystem(const qsv_state *st, int k, const int *qubits, int max_k, const char *what) {
    if (st->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs a qubit register");
    if (k < 1 || k > max_k || k > st->n)
        return qsv_fail(QSV_EINVAL, std::string(what) + ": keep between 1 and " + std::to_string(std::min(max_k, st->n)) + " qubits");
    if (st->n > SUB_MAX_QUBITS) return qsv_fail(QSV_EINVAL, std::string(what) + ": register too large");
    for (int i = 0; i < k; ++i) {
        if (qubits[i] < 0) return qsv_fail(QSV_EINVAL, "Non-negative index");
        if (qubits[i] >= st->n)
            return qsv_fail(QSV_EINVAL, "qubit index " + std::to_string(qubits[i]) + " out of range for a " + std::to_string(st->n) +
                                            "-qubit register");
        for (int j = 0; j < i; ++j)
            if (qubits[i] == qubits[j]) return qsv_fail(QSV_EINVAL, "Indices must be distinct.");
    }
    return QSV_OK;
}

}  // namespace

extern "C" {

int qsv_reduced_density_state(qsv_state *ket, int k, const int *qubits, qsv_state *rho) {
    if (!ket || !qubits || !rho) return qsv_fail(QSV_EINVAL, "null pointer");
    if (rho->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    int rc = check_subsystem(ket, k, qubits, SUB_MAX_K, "reduced state");
    if (rc) return rc;
    if (rho == ket) return qsv_fail(QSV_EINVAL, "the density register must not be the ket");
    if (rho->n != 2 * k) return qsv_fail(QSV_EINVAL, "the density register must have twice the kept qubits");
    if (rho->device != ket->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    if (!rho->owns_data) return qsv_fail(QSV_EINVAL, "the density register must be allocated by the library, not a view");
    rc = qsv_flush(ket);
    if (rc) return rc;
    rc = qsv_flush(rho);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(ket->device));
    if (rho->stream != ket->stream) QSV_HIP(hipStreamSynchronize(rho->stream));   // rho is overwritten: its own work first
    int bits[SUB_MAX_K];
    for (int j = 0; j < k; ++j) bits[j] = ket->n - 1 - qubits[j];
    const SubPlan p = sub_plan(ket->n, k, bits, ket->grid_cap);
    if (!p.ok) return qsv_fail(QSV_EINVAL, "reduced state: no plan for this shape");
    const dim3 bd(QSV_BLOCK);
    if (p.tiled) {
        rc = qsvk_ensure_matrix(ket, p.workspace_bytes);
        if (rc) return rc;
        double *partials = ket->dev_matrix;
        hipLaunchKernelGGL(k_subsys_tile, dim3(p.grid), bd, 0, ket->stream, static_cast<const amp_t *>(ket->data), p.g, partials);
        rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(k_subsys_finish, dim3(p.finish_grid), bd, 0, ket->stream, static_cast<const double *>(partials), p.g, rho->data);
        snprintf(ket->last_kernel, sizeof(ket->last_kernel), "k_subsys_tile");
    } else {
        hipLaunchKernelGGL(k_subsys_entry, dim3(p.grid), bd, 0, ket->stream, static_cast<const amp_t *>(ket->data), p.g, rho->data);
        snprintf(ket->last_kernel, sizeof(ket->last_kernel), "k_subsys_entry");
    }
    return check_launch();
}

int qsv_marginal_probabilities(qsv_state *st, int k, const int *qubits, double *out) {
    if (!st || !qubits || !out) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_subsystem(st, k, qubits, SUB_MARGINAL_MAX_K, "marginal probabilities");
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    int bits[SUB_MARGINAL_MAX_K];
    for (int j = 0; j < k; ++j) bits[j] = st->n - 1 - qubits[j];
    const MargPlan p = marginal_plan(st->n, k, bits);
    if (!p.ok) return qsv_fail(QSV_EINVAL, "marginal probabilities: no plan for this shape");
    rc = qsvk_ensure_matrix(st, p.workspace_bytes);
    if (rc) return rc;
    const uint64_t D = 1ull << k;
    const dim3 bd(QSV_BLOCK);
    double *d_out = st->dev_matrix;
    if (p.streaming) {
        double *partials = st->dev_matrix + D;
        hipLaunchKernelGGL(k_marginal_stream, dim3(p.grid), bd, 0, st->stream, static_cast<const amp_t *>(st->data), p.g, partials);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_marginal_stream");
        rc = check_launch();
        if (rc) return rc;
        rc = qsvk_sum_partials(st->stream, partials, static_cast<int>(p.g.waves), static_cast<int>(D), d_out);
        if (rc) return rc;
        std::vector<double> raw(D);                       // physical row order; at most 4096 entries in this form
        QSV_HIP(hipMemcpyAsync(raw.data(), d_out, sizeof(double) * D, hipMemcpyDeviceToHost, st->stream));
        QSV_HIP(hipStreamSynchronize(st->stream));
        for (uint64_t c = 0; c < D; ++c) out[c] = raw[sub_caller_row(p.g, static_cast<uint32_t>(c))];
        return QSV_OK;
    }
    hipLaunchKernelGGL(k_marginal_entry, dim3(p.grid), bd, 0, st->stream, static_cast<const amp_t *>(st->data), p.g, d_out);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_marginal_entry");
    rc = check_launch();
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * D, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

}  // extern "C"

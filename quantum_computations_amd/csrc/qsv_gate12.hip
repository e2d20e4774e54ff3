// 1- and 2-qubit gate kernels of the qubit register of libqsv.so, written for gfx950 (MI355X, wave64) only: dense and
// diagonal gates in the register forms (k_dense*, k_diag*) and the workgroup-tile form (k_dense_tile12*), with their
// launchers.  Wider dense gates are qsv_gatek.hip, gate sequences qsv_sequence.hip, the deferred-gate pass qsv_pass.hip,
// the staging ring, spare buffer and copy kernel qsv_state.hip.  Measurement, reshaping and reductions are
// qsv_readout.hip, Pauli strings qsv_pauli.hip.  The launch rules (items per thread, tile order, grid) are qsv_layout.h.
//
// Every gate is one streaming pass over the complex128 register in HBM: the path is bandwidth-bound
// (0.44-0.94 flop/B), so the kernels are organised around memory access, not arithmetic:
//   * a wave always touches 64 consecutive amplitudes (1 KiB) per load/store instruction: index bits 0..5 are
//     lane bits, whatever the target qubit;
//   * target bits >= 6 are resolved in registers (a thread owns the 2 or 4 amplitudes of its group);
//   * target bits < 6 lie inside a wavefront and are resolved with wave64 shuffles: each lane keeps its own
//     amplitude, fetches its partners' with __shfl_xor and computes only its own row of the matrix;
//   * control bits >= 6 are removed from the enumeration (amplitudes with control = 0 are never touched);
//     control bits < 6 predicate lanes;
//   * each thread keeps U independent work items in flight (8 x 16 B loads per lane) to cover HBM latency.
// This replaces Gate.apply -> expand_gate -> dense mat-vec of the reference
// (simulators/dv_simulator/gates.py:44-54, numpy_quantum.py:243-247).

#include "qsv_internal.h"
#include "qsv_device.h"
#include "qsv_layout.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace qsv_layout;   // the argument and record types of the kernels, and the host-side tables the launchers fill them from

static_assert(LANE_BITS == QSV_LANE_BITS && MAX_K == QSV_MAX_K && BLOCK == QSV_BLOCK, "qsv_layout.h and qsv_internal.h agree");

namespace {

// ----------------------------------------------------------------------------------------------------
// Dense 1- and 2-qubit gates (optionally controlled).
// ----------------------------------------------------------------------------------------------------
template <int KH, int KL, int U, bool NT>
__device__ __forceinline__ void dense_body(amp_t *__restrict__ a, const GateArgs &g) {
    constexpr int NH = 1 << KH, NL = 1 << KL, D = NH * NL;
    const int lane = threadIdx.x & 63;
    const bool lane_ok = (static_cast<uint32_t>(lane) & g.lane_ctrl) == g.lane_ctrl;

    // This lane's value of the low target bits.
    int l = 0;
#pragma unroll
    for (int j = 0; j < KL; ++j) l |= ((lane >> g.lbit[j]) & 1) << j;

    // coef[h][hp][x] = M[(h, l)][(hp, l ^ x)]: the matrix row(s) this lane computes.  For KL == 0 the
    // values are wave-uniform and stay in SGPRs; otherwise they are selected per lane once, up front.
    cplx coef[NH][NH][NL];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int hp = 0; hp < NH; ++hp)
#pragma unroll
            for (int x = 0; x < NL; ++x) {
                cplx c = {0.0, 0.0};
#pragma unroll
                for (int lc = 0; lc < NL; ++lc) {
                    const int row = (h << KL) | lc, col = (hp << KL) | (lc ^ x);
                    if (NL == 1 || l == lc) {
                        c.re = g.m[2 * (row * D + col)];
                        c.im = g.m[2 * (row * D + col) + 1];
                    }
                }
                coef[h][hp][x] = c;
            }

    constexpr uint64_t TILE = static_cast<uint64_t>(QSV_BLOCK) * U;
    const uint64_t ntiles = (g.W + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        amp_t v[U][NH];
        uint64_t base[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // the U items of a thread sit 2^ubit work items apart (ubit = 8: back to back tiles of 256)
            // tile order: with `remap` = R the launch walks R contiguous regions of the register side by side
            // (workgroups are dealt round-robin over the 8 XCDs, so R = 8 gives every XCD its own region)
            const uint64_t tile_eff = (g.remap > 1 && ntiles % g.remap == 0)
                                          ? (tile % g.remap) * (ntiles / g.remap) + tile / g.remap
                                          : tile;
            const uint64_t t = tile_eff * QSV_BLOCK + threadIdx.x;
            const uint64_t w = U == 1 ? t
                                      : (((t >> g.ubit) * U + u) << g.ubit) | (t & ((1ull << g.ubit) - 1ull));
            ok[u] = w < g.W;  // W is a multiple of 64: uniform over the wave
            base[u] = deposit(w, g);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                v[u][h] = amp_t{0.0, 0.0};
                if (ok[u] && lane_ok) v[u][h] = ld<NT>(a + base[u] + g.hoff[h]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            amp_t out[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) out[h] = amp_t{0.0, 0.0};
#pragma unroll
            for (int x = 0; x < NL; ++x)
#pragma unroll
                for (int hp = 0; hp < NH; ++hp) {
                    const amp_t p = (x == 0) ? v[u][hp] : shfl_xor_amp(v[u][hp], g.lxor[x]);
#pragma unroll
                    for (int h = 0; h < NH; ++h) out[h] = cfma(coef[h][hp][x], p, out[h]);
                }
            if (lane_ok) {
#pragma unroll
                for (int h = 0; h < NH; ++h) st<NT>(a + base[u] + g.hoff[h], out[h]);
            }
        }
    }
}

// k_dense: every amplitude is read and written once (2 * 16 * 2^n bytes).  k_dense_ctrl: the same body on a
// sub-space (controlled gates, SWAP as a pair exchange) -- a separate symbol so that profiles keep the
// full-traffic launches apart from the reduced-traffic ones.
template <int KH, int KL, int U, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_dense(amp_t *__restrict__ a, const GateArgs g) {
    dense_body<KH, KL, U, NT>(a, g);
}

template <int KH, int KL, int U, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_dense_ctrl(amp_t *__restrict__ a, const GateArgs g) {
    dense_body<KH, KL, U, NT>(a, g);
}

// ----------------------------------------------------------------------------------------------------
// Diagonal gates: one multiply per touched amplitude, natural (fully coalesced) enumeration.
// ----------------------------------------------------------------------------------------------------
template <int U, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag(amp_t *__restrict__ a, const DiagArgs g) {
    const int lane = threadIdx.x & 63;
    const bool lane_ok = (static_cast<uint32_t>(lane) & g.lane_ctrl) == g.lane_ctrl;
    const cplx d0 = {g.d[0], g.d[1]}, d1 = {g.d[2], g.d[3]}, d2 = {g.d[4], g.d[5]}, d3 = {g.d[6], g.d[7]};
    constexpr uint64_t TILE = static_cast<uint64_t>(QSV_BLOCK) * U;
    const uint64_t ntiles = (g.W + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        amp_t v[U];
        uint64_t idx[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t tile_eff = (g.remap > 1 && ntiles % g.remap == 0)
                                          ? (tile % g.remap) * (ntiles / g.remap) + tile / g.remap
                                          : tile;
            const uint64_t w = tile_eff * TILE + static_cast<uint64_t>(u) * QSV_BLOCK + threadIdx.x;
            ok[u] = (w < g.W) && lane_ok;
            idx[u] = deposit(w, g);
            if (ok[u]) v[u] = ld<NT>(a + idx[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const int s0 = static_cast<int>((idx[u] >> g.b0) & 1ull);
            cplx d;
            if (g.b1 < 0) {
                d = s0 ? d1 : d0;
            } else {
                const int s1 = static_cast<int>((idx[u] >> g.b1) & 1ull);
                d = s0 ? (s1 ? d3 : d2) : (s1 ? d1 : d0);
            }
            st<NT>(a + idx[u], cmul_diag(d, v[u]));
        }
    }
}

// Generic-K diagonal: table of 2^K complex numbers in device memory, staged through LDS.
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_table(amp_t *__restrict__ a, uint64_t amps, int K,
                                                         const uint8_t *__restrict__ bitpos /*K, device*/,
                                                         const double *__restrict__ table) {
    __shared__ double tab[2 << QSV_MAX_K];
    __shared__ int bp[QSV_MAX_K];
    for (int i = threadIdx.x; i < (2 << K); i += blockDim.x) tab[i] = table[i];
    if (threadIdx.x < K) bp[threadIdx.x] = bitpos[threadIdx.x];
    __syncthreads();
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        int sel = 0;
        for (int j = 0; j < K; ++j) sel |= static_cast<int>((i >> bp[j]) & 1ull) << (K - 1 - j);
        const cplx d = {tab[2 * sel], tab[2 * sel + 1]};
        a[i] = cmul(d, a[i]);
    }
}

// K-qubit diagonal (K <= 6): a[i] *= table[bits of i at bitpos], natural order, table in LDS.
template <int ITEMS>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_table_s(amp_t *__restrict__ a, uint64_t amps, int K,
                                                           const uint8_t *__restrict__ bitpos,
                                                           const double *__restrict__ table) {
    __shared__ amp_t tab[1 << QSV_MAX_K];
    __shared__ int bp[QSV_MAX_K];
    if (threadIdx.x < (1 << K)) tab[threadIdx.x] = amp_t{table[2 * threadIdx.x], table[2 * threadIdx.x + 1]};
    if (threadIdx.x < K) bp[threadIdx.x] = bitpos[threadIdx.x];
    __syncthreads();
    const uint64_t i0 = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) * ITEMS + threadIdx.x;
    amp_t v[ITEMS];
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) v[u] = __builtin_nontemporal_load(a + i0 + u * QSV_BLOCK);
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
        const uint64_t i = i0 + u * QSV_BLOCK;
        int sel = 0;
        for (int j = 0; j < K; ++j) sel |= static_cast<int>((i >> bp[j]) & 1ull) << (K - 1 - j);
        const amp_t d = tab[sel];
        __builtin_nontemporal_store(cmul(cplx{d.x, d.y}, v[u]), a + i);
    }
}

// ----------------------------------------------------------------------------------------------------
// host-side helpers
// ----------------------------------------------------------------------------------------------------
LaunchOptions launch_options(const qsv_state *st) {
    return LaunchOptions{st->unroll, st->remap, st->ubit, st->grid_cap};
}

// The launch rules are qsv_layout::dense_launch / diag_launch; what stays here is the launch itself.  U = 1, 2, 4, 8 are
// built, any other value runs as 8 (with_pow2).
template <int KH, int KL>
int launch_dense(qsv_state *st, const GateArgs &g) {
    const bool sub = g.nins > KH || g.lane_ctrl != 0, nt = st->nontemporal != 0;
    // the address bit of high target i, as the kernel sees it: the top set bit of hoff[1 << i] (a pair exchange: of hoff[1])
    int hbit[2] = {0, 0};
    for (int i = 0; i < KH; ++i) hbit[i] = 63 - __builtin_clzll(g.hoff[1 << i] | 1);
    const Launch12 l = dense_launch(KH, KL, hbit, sub, g.W, launch_options(st));
    GateArgs ga = g;
    ga.ubit = l.ubit;
    ga.remap = l.remap;
    const dim3 gd(l.grid), bd(QSV_BLOCK);
    with_pow2<1, 8>(l.U, [&](auto U) {
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense%s<%d, %d, %d, %s>", sub ? "_ctrl" : "", KH, KL, U.value,
                 nt ? "true" : "false");
        with_bool(nt, [&](auto NT) {
            if (sub) hipLaunchKernelGGL((k_dense_ctrl<KH, KL, U.value, NT.value>), gd, bd, 0, st->stream, st->data, ga);
            else hipLaunchKernelGGL((k_dense<KH, KL, U.value, NT.value>), gd, bd, 0, st->stream, st->data, ga);
        });
    });
    return check_launch();
}

int launch_diag(qsv_state *st, const DiagArgs &g0) {
    const bool sub = g0.nins > 0 || g0.lane_ctrl != 0, nt = st->nontemporal != 0;
    const Launch12 l = diag_launch(sub, g0.W, launch_options(st));
    DiagArgs g = g0;
    g.remap = l.remap;
    const dim3 gd(l.grid), bd(QSV_BLOCK);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag<%d, %s>%s", l.U, nt ? "true" : "false", sub ? " [sub-space]" : "");
    with_pow2<1, 8>(l.U, [&](auto U) { with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_diag<U.value, NT.value>), gd, bd, 0, st->stream, st->data, g);
    }); });
    return check_launch();
}

int dispatch_dense(qsv_state *st, int KH, int KL, const GateArgs &g) {
    if (KH == 1 && KL == 0) return launch_dense<1, 0>(st, g);
    if (KH == 0 && KL == 1) return launch_dense<0, 1>(st, g);
    if (KH == 2 && KL == 0) return launch_dense<2, 0>(st, g);
    if (KH == 1 && KL == 1) return launch_dense<1, 1>(st, g);
    if (KH == 0 && KL == 2) return launch_dense<0, 2>(st, g);
    return qsv_fail(QSV_EINVAL, "dense kernel: unsupported target split");
}

// Fill pos/or_mask/lane_ctrl/W from target and control bit positions.
template <class Args>
int fill_enumeration(const qsv_state *st, Args &g, const std::vector<int> &removed_high, int nctrl,
                     const int *cbits) {
    std::vector<int> ins(removed_high);
    g.or_mask = 0;
    g.lane_ctrl = 0;
    for (int i = 0; i < nctrl; ++i) {
        if (cbits[i] >= QSV_LANE_BITS) {
            ins.push_back(cbits[i]);
            g.or_mask |= 1ull << cbits[i];
        } else {
            g.lane_ctrl |= 1u << cbits[i];
        }
    }
    std::sort(ins.begin(), ins.end());
    if (ins.size() > static_cast<size_t>(QSV_MAX_INS)) return qsv_fail(QSV_EINVAL, "too many controls");
    g.nins = static_cast<int>(ins.size());
    for (size_t i = 0; i < ins.size(); ++i) g.pos[i] = static_cast<uint32_t>(ins[i]);
    g.W = st->amps >> ins.size();
    return QSV_OK;
}

// Expand a controlled k-qubit matrix to the full (k + nctrl)-qubit matrix (controls as leading legs).
std::vector<double> expand_controls(int k, int nctrl, const double *m) {
    const int D = 1 << k, F = 1 << (k + nctrl);
    std::vector<double> full(2ull * F * F, 0.0);
    for (int r = 0; r < F; ++r) full[2 * (r * F + r)] = 1.0;
    const int b0 = F - D;  // all controls = 1
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            full[2 * ((b0 + r) * F + b0 + c)] = m[2 * (r * D + c)];
            full[2 * ((b0 + r) * F + b0 + c) + 1] = m[2 * (r * D + c) + 1];
        }
    return full;
}

}  // namespace

// 1- and 2-qubit gates in the same form: one wave per input row (2 / 4 waves per workgroup), the matrix and the row
// offsets in the kernel arguments.  On the benchmark circuit's placements 4-8 % faster than the register form (k_dense):
// 1.28-1.34 ms against 1.31-1.48 per 1-qubit gate at n = 28, 1.36 against 1.48 on average over all pairs of bits >= 6.

template <int K, bool NT>
__device__ __forceinline__ void tile12_body(amp_t *__restrict__ a, const BigArgs &g, const SmallGate &sg) {
    constexpr int D = 1 << K;
    __shared__ amp_t tile[D * 64];
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    amp_t *p = a + deposit(g.w0 + tile_id * 64 + lane, g) + sg.off[q];
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
    __builtin_amdgcn_global_load_lds(p, tile + q * 64, 16, 0, NT ? 2 : 0);
#endif
    __syncthreads();
    amp_t acc = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < D; ++c)
        acc = cfma(cplx{sg.m[2 * (q * D + c)], sg.m[2 * (q * D + c) + 1]}, tile[c * 64 + lane], acc);
    if (NT) __builtin_nontemporal_store(acc, p);
    else *p = acc;
}

template <int K, bool NT>
__global__ __launch_bounds__((1 << K) * 64) void k_dense_tile12(amp_t *__restrict__ a, const BigArgs g, const SmallGate sg) {
    tile12_body<K, NT>(a, g, sg);
}

// the same body on a sub-space (controls removed from the enumeration and forced to 1): a symbol of its own, so that
// profiles keep full- and reduced-traffic launches apart (as k_dense / k_dense_ctrl do)
template <int K, bool NT>
__global__ __launch_bounds__((1 << K) * 64) void k_dense_tile12_ctrl(amp_t *__restrict__ a, const BigArgs g, const SmallGate sg) {
    tile12_body<K, NT>(a, g, sg);
}

// the dispatches of one tile-form gate (registers beyond 2^24 tiles take several); `sub`: the reduced-traffic symbol
static int launch_tile12_kernels(qsv_state *st, int k, bool sub, BigArgs g, const SmallGate &sg) {
    const bool nt = st->nontemporal != 0;
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_tile12%s<%d, %s>", sub ? "_ctrl" : "", k, nt ? "true" : "false");
    return launch_ranges(g, DISPATCH_TILES * 64, [&](uint64_t columns) {
        const dim3 gd(static_cast<unsigned>(columns / 64)), bd((1 << k) * 64);
        with_bool(nt, [&](auto NT) {
            if (sub) hipLaunchKernelGGL((k_dense_tile12_ctrl<1, NT.value>), gd, bd, 0, st->stream, st->data, g, sg);
            else if (k == 1) hipLaunchKernelGGL((k_dense_tile12<1, NT.value>), gd, bd, 0, st->stream, st->data, g, sg);
            else hipLaunchKernelGGL((k_dense_tile12<2, NT.value>), gd, bd, 0, st->stream, st->data, g, sg);
        });
    });
}

static int launch_tile12(qsv_state *st, int k, const int *bits, int nctrl, const int *cbits, const double *m_user) {
    if (!tile12_takes(st->amps, k, bits, nctrl, cbits)) return QSV_UNHANDLED_KQ;
    SmallGate sg;    // kernel index bit i <-> leg i
    std::memset(&sg, 0, sizeof(sg));
    const std::vector<uint64_t> off = offsets(std::vector<int>(bits, bits + k));
    std::copy(off.begin(), off.end(), sg.off);
    write_matrix(MAT_COMPLEX, 1 << k, m_user, user_index(k, bits, bits).data(), sg.m);
    std::vector<int> sorted(bits, bits + k);
    std::sort(sorted.begin(), sorted.end());
    std::vector<int> ins(sorted);
    ins.insert(ins.end(), cbits, cbits + nctrl);
    uint64_t or_mask = 0;
    for (int i = 0; i < nctrl; ++i) or_mask |= 1ull << cbits[i];
    BigArgs g = with_enumeration<BigArgs>(enumeration(st->amps >> (k + nctrl), ins, or_mask));
    // controlled launches (CX on 40 random control / target pairs: 0.686 ms with 8 regions, 0.734 for k_dense_ctrl)
    g.regions = regions_or(st, nctrl ? 8 : tile_regions(k, sorted));
    return launch_tile12_kernels(st, k, nctrl != 0, g, sg);
}

// bits[j] = bit position of matrix leg j (leg 0 most significant); k in {1, 2}.
int qsvk_dense(qsv_state *st, int k, const int *bits, int nctrl, const int *cbits, const double *m_user) {
    if (k < 1 || k > 2) return qsv_fail(QSV_EINVAL, "dense kernel handles 1- and 2-qubit matrices");
    if (st->n < QSV_LANE_BITS) {
        // tiny register: fold the controls into a (k + nctrl)-qubit matrix for the gather kernel
        if (nctrl == 0) return qsvk_generic(st, k, bits, m_user);
        std::vector<int> legs(cbits, cbits + nctrl);
        legs.insert(legs.end(), bits, bits + k);
        const std::vector<double> full = expand_controls(k, nctrl, m_user);
        return qsvk_generic(st, k + nctrl, legs.data(), full.data());
    }
    // dense, every target on bit 3 (1 qubit) / 6 (2 qubits) or higher, controls on bit 3 or higher: the workgroup-tile
    // form (k_dense_tile12 / k_dense_tile12_ctrl); QSV_OPT_KQ_VARIANT 1 or 2, or an explicit QSV_OPT_UNROLL, keep k_dense
    if (st->unroll == 0 && st->kq_variant != 1 && st->kq_variant != 2) {
        const int rc_tile = launch_tile12(st, k, bits, nctrl, cbits, m_user);
        if (rc_tile != QSV_UNHANDLED_KQ) return rc_tile;
    }
    GateArgs g;
    std::memset(&g, 0, sizeof(g));
    std::vector<int> high, low;
    for (int j = 0; j < k; ++j) (bits[j] >= QSV_LANE_BITS ? high : low).push_back(bits[j]);
    const int KH = static_cast<int>(high.size()), KL = static_cast<int>(low.size());
    int rc = fill_enumeration(st, g, high, nctrl, cbits);
    if (rc) return rc;
    const std::vector<uint64_t> hoff = offsets(high), lxor = offsets(low);
    std::copy(hoff.begin(), hoff.end(), g.hoff);
    std::copy(lxor.begin(), lxor.end(), g.lxor);   // lane xor mask of low-bit combination x
    for (int j = 0; j < KL; ++j) g.lbit[j] = low[j];
    // kernel order: index = (h << KL) | l, h bit i <-> high[i], l bit i <-> low[i]
    std::vector<int> kb(low);
    kb.insert(kb.end(), high.begin(), high.end());
    write_matrix(MAT_COMPLEX, 1 << k, m_user, user_index(k, bits, kb.data()).data(), g.m);
    return dispatch_dense(st, KH, KL, g);
}

// SWAP of two bits >= QSV_LANE_BITS: exchange a[base | Sa] <-> a[base | Sb]; the 00 and 11 quarters stay put.
int qsvk_pair_exchange(qsv_state *st, int bit_a, int bit_b) {
    const uint64_t quarter = st->amps >> 2;
    if (st->unroll == 0 && st->kq_variant != 1 && st->kq_variant != 2 && bit_a >= 3 && bit_b >= 3 && quarter >= 64 &&
        quarter % 64 == 0) {
        // tile form: an X "gate" between the amplitudes with (a, b) = (1, 0) and (0, 1); both bits leave the enumeration
        SmallGate sg;
        std::memset(&sg, 0, sizeof(sg));
        sg.m[2] = 1.0;   // m[0][1]
        sg.m[4] = 1.0;   // m[1][0]
        sg.off[0] = 1ull << bit_a;
        sg.off[1] = 1ull << bit_b;
        BigArgs t = with_enumeration<BigArgs>(enumeration(quarter, {bit_a, bit_b}));
        t.regions = regions_or(st, 8);
        return launch_tile12_kernels(st, 1, true, t, sg);
    }
    GateArgs g;
    std::memset(&g, 0, sizeof(g));
    std::vector<int> removed = {bit_a, bit_b};
    int rc = fill_enumeration(st, g, removed, 0, nullptr);
    if (rc) return rc;
    g.hoff[0] = 1ull << bit_a;
    g.hoff[1] = 1ull << bit_b;
    const double x[8] = {0, 0, 1, 0, 1, 0, 0, 0};
    std::memcpy(g.m, x, sizeof(x));
    return dispatch_dense(st, 1, 0, g);
}

// bits[j] = position of diagonal leg j (leg 0 most significant); d has 2^k complex entries.
int qsvk_diag(qsv_state *st, int k, const int *bits, int nctrl, const int *cbits, const double *d_user) {
    if (k < 1 || k > QSV_MAX_K) return qsv_fail(QSV_EINVAL, "diagonal gate: k must be in 1..6");
    if (k <= 2 && st->n >= QSV_LANE_BITS) {
        DiagArgs g;
        std::memset(&g, 0, sizeof(g));
        int rc = fill_enumeration(st, g, {}, nctrl, cbits);
        if (rc) return rc;
        g.b0 = bits[0];
        g.b1 = k == 2 ? bits[1] : -1;
        std::memcpy(g.d, d_user, sizeof(double) * (2 << k));
        return launch_diag(st, g);
    }
    // table path (k > 2 or tiny register); controls are folded into the table
    std::vector<int> legs(cbits, cbits + nctrl);
    legs.insert(legs.end(), bits, bits + k);
    const int K = k + nctrl;
    if (K > QSV_MAX_K) return qsv_fail(QSV_EINVAL, "diagonal gate: too many legs for the table kernel");
    std::vector<double> table(2ull << K, 0.0);
    for (int i = 0; i < (1 << K); ++i) {
        table[2 * i] = 1.0;
        if ((i >> k) == (1 << nctrl) - 1) {
            table[2 * i] = d_user[2 * (i & ((1 << k) - 1))];
            table[2 * i + 1] = d_user[2 * (i & ((1 << k) - 1)) + 1];
        }
    }
    const size_t tbytes = sizeof(double) * table.size();
    uint8_t pos[8] = {0};
    for (int j = 0; j < K; ++j) pos[j] = static_cast<uint8_t>(legs[j]);
    StageRef staged;
    int rc = qsvk_stage(st, table.data(), tbytes, pos, 8, &staged);
    if (rc) return rc;
    const double *dtable = reinterpret_cast<const double *>(staged.dev);
    const uint8_t *dpos = reinterpret_cast<const uint8_t *>(staged.dev + qsv_pad16(tbytes));
    if (streaming_forms(st)) {
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag_table_s");
        with_pow2<1, 4>(ro_fit_items(getenv("QSV_RO_ITEMS") ? ro_move_items() : 2, st->amps), [&](auto IT) {
            hipLaunchKernelGGL(k_diag_table_s<IT.value>, dim3(static_cast<unsigned>(st->amps / (QSV_BLOCK * IT.value))), dim3(QSV_BLOCK), 0,
                               st->stream, st->data, st->amps, K, dpos, dtable);
        });
    } else {
        const int grid = grid_for(st->amps, QSV_BLOCK, 4096);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag_table");
        hipLaunchKernelGGL(k_diag_table, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, K, dpos, dtable);
    }
    rc = check_launch();
    if (rc) return rc;
    return qsvk_stage_done(st, staged);
}

int qsvk_phase(qsv_state *st, int nctrl, const int *cbits, double re, double im) {
    if (st->n < QSV_LANE_BITS || nctrl == 0) {
        if (nctrl == 0) return qsvk_scale(st, re, im);
        if (nctrl > QSV_MAX_K) return qsv_fail(QSV_EINVAL, "phase on a tiny register: too many qubits");
        // all qubits are "controls": table with the phase at the all-ones entry
        std::vector<double> d = {1.0, 0.0, re, im};
        return qsvk_diag(st, 1, cbits + nctrl - 1, nctrl - 1, cbits, d.data());
    }
    DiagArgs g;
    std::memset(&g, 0, sizeof(g));
    int rc = fill_enumeration(st, g, {}, nctrl, cbits);
    if (rc) return rc;
    // every enumerated amplitude already has all controls = 1: multiply by the phase whatever bit b0 is
    g.b0 = 0;
    g.b1 = -1;
    g.d[0] = g.d[2] = re;
    g.d[1] = g.d[3] = im;
    return launch_diag(st, g);
}

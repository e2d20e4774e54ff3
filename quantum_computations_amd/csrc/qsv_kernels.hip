// Gate kernels of the qubit register of libqsv.so, written for gfx950 (MI355X, wave64) only, with the state plumbing
// (staging ring, spare buffer, copy).  Measurement, reshaping and reductions are qsv_readout.hip, Pauli strings qsv_pauli.hip.
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
#include "qsv_plan.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <type_traits>
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

// ----------------------------------------------------------------------------------------------------
// Generic k-qubit dense gate (k <= 6) and the tiny-register path (n < 6): one thread per group, gathers
// with arbitrary strides.  Correct for every layout; not bandwidth-tuned (DESIGN.md "kernels").
// ----------------------------------------------------------------------------------------------------
struct GenericArgs {
    uint64_t W;
    int32_t K;
    uint8_t sorted_pos[QSV_MAX_K];  // ascending target bit positions (for deposit)
    uint8_t leg_pos[QSV_MAX_K];     // bit position of matrix leg j (leg 0 = most significant)
};

template <int K>
__global__ __launch_bounds__(QSV_BLOCK) void k_generic(amp_t *__restrict__ a, const GenericArgs g,
                                                      const double *__restrict__ M) {
    constexpr int D = 1 << K;
    uint64_t off[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        uint64_t o = 0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if ((c >> (K - 1 - j)) & 1) o |= 1ull << g.leg_pos[j];
        off[c] = o;
    }
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; w < g.W;
         w += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        uint64_t base = w;
#pragma unroll
        for (int j = 0; j < K; ++j) base = insert_zero(base, g.sorted_pos[j]);
        amp_t in[D];
#pragma unroll
        for (int c = 0; c < D; ++c) in[c] = a[base + off[c]];
#pragma unroll 1
        for (int r = 0; r < D; ++r) {
            amp_t acc = {0.0, 0.0};
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const cplx m = {M[2 * (r * D + c)], M[2 * (r * D + c) + 1]};
                acc = cfma(m, in[c], acc);
            }
            // rows are written as they are produced: all inputs are already in registers
            uint64_t o = 0;
            for (int j = 0; j < K; ++j)
                if ((r >> (K - 1 - j)) & 1) o |= 1ull << g.leg_pos[j];
            a[base + o] = acc;
        }
    }
}

// ----------------------------------------------------------------------------------------------------
// Register-blocked k-qubit dense gate (k = 3..5: fused gate blocks, Gate(indices, matrix) with many legs).
// A thread owns the 2^k amplitudes of one group in registers (k = 5: 128 VGPRs), the six lowest NON-target bits
// are the lane bits, rows are produced one at a time with the matrix read through scalar loads (wave-uniform
// addresses -> s_load_dwordx16, no LDS) and stored in place.  2^k complex FMAs per amplitude: k = 5 is
// 8 flop/B, close to the fp64 ridge of the chip, so this kernel is bounded by HBM *and* the fp64 pipe.
// Device table layout behind M: [2^k x 2^k complex matrix][2^k uint64 amplitude offsets].
// ----------------------------------------------------------------------------------------------------
//
// Target bits below 6 (KL of them) are lane bits, and a wave must keep touching 64 consecutive amplitudes per
// instruction.  So the thread loads 2^k coalesced amplitudes over the KH high targets and KL *stand-in* high
// bits E_j instead, and the wave then swaps the roles of lane bit L_j and register bit e_j with KL butterfly
// stages of wave64 shuffles (a distributed transpose): afterwards every thread holds one complete group.  The
// same stages, applied to the outputs, restore the memory layout before the coalesced stores.

template <int D, int KL>
__device__ __forceinline__ void wave_transpose(amp_t (&x)[D], const BigArgs &g, int lane) {
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        const int lb = g.lbit[j];
        const bool up = (lane >> lb) & 1;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            if (c & (1 << j)) continue;
            const amp_t r0 = x[c], r1 = x[c | (1 << j)];
            const amp_t recv = shfl_xor_amp(up ? r0 : r1, 1 << lb);  // I keep entry e_j == my bit, trade the other
            x[c] = up ? recv : r0;
            x[c | (1 << j)] = up ? r1 : recv;
        }
    }
}

// Complex matrix rows in three real multiplications per entry instead of four ("3M"): with As = Ar + Ai prepared by the
// host and xs = xr + xi formed once per input amplitude,
//     S1 = sum Ar xr,  S2 = sum Ai xi,  S3 = sum As xs   ->   re = S1 - S2,  im = S3 - S1 - S2.
// A 32 x 32 complex product per amplitude is 8 flop/B -- at the chip's fp64 ridge -- so a quarter fewer FMAs is time
// (round 3; normwise error bound as for the four-multiplication form).  A row of the matrix is three planes of D doubles.
template <int D>
__device__ __forceinline__ amp_t row_product_3m(const double *__restrict__ row, const amp_t (&x)[D], const double (&xs)[D]) {
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        s1 = fma(row[c], x[c].x, s1);
        s2 = fma(row[D + c], x[c].y, s2);
        s3 = fma(row[2 * D + c], xs[c], s3);
    }
    return amp_t{s1 - s2, s3 - s1 - s2};
}

template <int K, int KL, bool NT, bool M3 = false>
__global__ __launch_bounds__(QSV_BLOCK) void k_dense_big(amp_t *__restrict__ a, const BigArgs g,
                                                        const double *__restrict__ M,
                                                        const uint64_t *__restrict__ hoff) {
    constexpr int D = 1 << K;
    // straight-line body (a grid-stride loop here cost the k = 5 transposed variants 4x: registers live across
    // the back edge); registers beyond 2^32 work items are covered by several launches with a work-item offset
    // tile order as in k_dense: `regions` contiguous pieces of this launch's range walked side by side
    const uint64_t tile = (g.regions > 1 && gridDim.x % g.regions == 0)
                              ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                              : blockIdx.x;
    const uint64_t w = g.w0 + tile * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (w >= g.W) return;  // W and w0 are multiples of 64 whenever KL > 0: whole waves leave together
    const uint64_t base = deposit(w, g);
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    if constexpr (KL == 0) {
        double xs[M3 ? D : 1];
        if constexpr (M3) {
#pragma unroll
            for (int c = 0; c < D; ++c) xs[c] = x[c].x + x[c].y;
        }
#pragma unroll 1
        for (int r = 0; r < D; ++r) {
            amp_t acc = {0.0, 0.0};
            if constexpr (M3) {
                acc = row_product_3m<D>(M + 3 * D * r, x, xs);
            } else {
                const double *row = M + 2 * D * r;
#pragma unroll
                for (int c = 0; c < D; ++c) acc = cfma(cplx{row[2 * c], row[2 * c + 1]}, x[c], acc);
            }
            st<NT>(a + base + hoff[r], acc);  // in place: every input of this group is already in registers
        }
    } else {
        static_assert(!M3, "the shuffle form keeps two register arrays: no room for a third");
        const int lane = threadIdx.x & 63;
        wave_transpose<D, KL>(x, g, lane);
        amp_t y[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const double *row = M + 2 * D * r;
            amp_t acc = {0.0, 0.0};
#pragma unroll
            for (int c = 0; c < D; ++c) acc = cfma(cplx{row[2 * c], row[2 * c + 1]}, x[c], acc);
            y[r] = acc;
        }
        wave_transpose<D, KL>(y, g, lane);
#pragma unroll
        for (int c = 0; c < D; ++c) st<NT>(a + base + hoff[c], y[c]);
    }
}


// ----------------------------------------------------------------------------------------------------
// Register-blocked k-qubit dense gate with target bits below 6, second form: the low target bits are brought into
// registers WITHOUT wave shuffles and without a second register array for the results.
//
// A low target bit L still gets a stand-in high bit E (as above), so that whatever a wave-instruction touches is made
// of whole 128-byte lines.  But only the bits 0..2 of the index live INSIDE a line.  For a target on lane bit 3, 4 or
// 5 ("A" bits) the exchange of roles between L and E is pure address arithmetic: lane l fetches, for register value
// v, the amplitude in row E := (bit L of l), column (l with bit L := v).  Each wave-instruction then reads 8 whole
// lines from 2^|A| rows instead of 8 consecutive ones -- the same number of lines -- and the thread owns both values
// of bit L at once.  Nothing moves between lanes.
// Targets on lane bits 0..2 ("B" bits, at most three) need a real transpose among the 2^|B| neighbouring lanes that
// share a line.  It goes through LDS, 2^|B| rows of 64 amplitudes (at most 8 KiB per wave) at a time: lane l writes
// row s at column l ^ dep(s) and reads row (its own B bits) at column l ^ dep(t) -- an XOR swizzle that makes both
// directions conflict-free for 16-byte accesses (a 16-lane group of ds_read_b128 always sees 16 different columns
// mod 16, and rows are 64 slots apart).  Results take the same road back one row group at a time, straight from the
// accumulator, so the thread holds the 2^K inputs (K = 5: 128 VGPRs) and nothing else: 3 waves per SIMD instead of
// one, and the next wave's loads overlap this wave's arithmetic.
// ----------------------------------------------------------------------------------------------------

// The LDS rows are private to a wave (a wave exchanges data with itself only), and the LDS executes one wave's
// instructions in order: no workgroup barrier is needed, only the compiler must keep the program order of the
// accesses (it does: they may alias) -- wave_sync() marks the spots.
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

template <int K, int KB, bool NT, bool REALM, int BLOCK, bool M3 = false>
__global__ __launch_bounds__(BLOCK) void k_dense_lds(amp_t *__restrict__ a, const LdsArgs g,
                                                     const double *__restrict__ M,
                                                     const uint64_t *__restrict__ hoff) {
    constexpr int D = 1 << K, NB = 1 << KB;
    __shared__ amp_t tiles[KB > 0 ? NB * BLOCK : 1];
    amp_t *tile = tiles + (KB > 0 ? NB * 64 * (threadIdx.x >> 6) : 0);
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    const uint64_t w = g.w0 + tile_id * static_cast<uint64_t>(BLOCK) + threadIdx.x;
    if (w >= g.W) return;  // W and w0 are multiples of 64: whole waves leave together
    const uint32_t lane = threadIdx.x & 63;
    // row of this lane: its A bits move from the column to the stand-in bits
    uint64_t base = deposit(w, g) & ~static_cast<uint64_t>(g.amask);
    for (int j = 0; j < g.na; ++j) base |= static_cast<uint64_t>((lane >> g.abit[j]) & 1u) << g.aE[j];
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    uint32_t my_row = 0;  // this lane's B bits, as a row number
    if constexpr (KB > 0) {
#pragma unroll
        for (int v = 1; v < NB; ++v)
            if ((lane & g.bmask) == g.bdep[v]) my_row = v;
#pragma unroll
        for (int o = 0; o < D / NB; ++o) {
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) tile[s * 64 + (lane ^ g.bdep[s])] = x[o * NB + s];
            wave_sync();
#pragma unroll
            for (int t = 0; t < NB; ++t) x[o * NB + t] = tile[my_row * 64 + (lane ^ g.bdep[t])];
        }
    }
    // every thread now owns one complete group; rows of the matrix come through scalar loads
    double xs[M3 ? D : 1];
    if constexpr (M3) {
        static_assert(!REALM, "a real matrix needs two multiplications per entry anyway");
#pragma unroll
        for (int c = 0; c < D; ++c) xs[c] = x[c].x + x[c].y;
    }
#pragma unroll 1
    for (int o = 0; o < D / NB; ++o) {
        if constexpr (KB > 0) wave_sync();
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int r = o * NB + t;
            amp_t acc = {0.0, 0.0};
            if constexpr (M3) {
                acc = row_product_3m<D>(M + 3 * D * r, x, xs);
            } else if constexpr (REALM) {
                const double *row = M + D * r;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    acc.x = fma(row[c], x[c].x, acc.x);
                    acc.y = fma(row[c], x[c].y, acc.y);
                }
            } else {
                const double *row = M + 2 * D * r;
#pragma unroll
                for (int c = 0; c < D; ++c) acc = cfma(cplx{row[2 * c], row[2 * c + 1]}, x[c], acc);
            }
            if constexpr (KB > 0) tile[my_row * 64 + (lane ^ g.bdep[t])] = acc;
            else st<NT>(a + base + hoff[r], acc);  // in place: every input of this group is already in registers
        }
        if constexpr (KB > 0) {
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) st<NT>(a + base + hoff[o * NB + s], tile[s * 64 + (lane ^ g.bdep[s])]);
        }
    }
}


// ----------------------------------------------------------------------------------------------------
// Fused 5-qubit blocks as a SEQUENCE of their source gates (round 3).  A dense 32 x 32 complex block costs 4 x 1024 real
// FMAs per amplitude group -- the one shape of the gate path that is bound by arithmetic (the vector pipe is 81 % busy at
// the clock its power draw leaves it: profiles/r03_k5_sq_counters.txt).  But a fused block IS a product of a few 1- and
// 2-qubit gates (5.9 on average on the benchmark circuit): applied one after the other to the 32 amplitudes a thread
// already holds in registers they cost 256 FMAs per 1-qubit gate and 512 per 2-qubit gate, ~2 400 per block instead of
// 4 096, and nothing but the gates' own small matrices comes through the scalar cache.  Loads, the exchange of low target bits
// (address arithmetic for lane bits 3..5, the XOR-swizzled LDS rows for bits 0..2) and stores are k_dense_big's /
// k_dense_lds's; only the arithmetic in the middle differs.  The register index is runtime data of the gate list, the
// register ARRAY must be indexed statically: one unrolled body per register bit (1-qubit gates) and per pair of register
// bits (2-qubit gates, leg 0 canonicalised onto the higher bit by the host), selected by a wave-uniform switch.
// ----------------------------------------------------------------------------------------------------
static int seq_max_work() {
    static const int v = [] {
        const char *e = getenv("QSV_SEQUENCE_WORK");
        return e ? atoi(e) : 0;      // measured (profiles/r03_sequence_blocks.txt): no faster than the dense block
    }();
    return v;
}

template <int J, int D = 32>
__device__ __forceinline__ void seq_apply1(amp_t (&x)[D], const double *__restrict__ m) {
    const cplx m00{m[0], m[1]}, m01{m[2], m[3]}, m10{m[4], m[5]}, m11{m[6], m[7]};
#pragma unroll
    for (int c = 0; c < D; ++c) {
        if (c & (1 << J)) continue;
        const amp_t a0 = x[c], a1 = x[c | (1 << J)];
        x[c] = cfma(m01, a1, cmul(m00, a0));
        x[c | (1 << J)] = cfma(m11, a1, cmul(m10, a0));
    }
}

template <int HI, int LO, int D = 32>
__device__ __forceinline__ void seq_apply2(amp_t (&x)[D], const double *__restrict__ m) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
        if (c & ((1 << HI) | (1 << LO))) continue;
        const amp_t in[4] = {x[c], x[c | (1 << LO)], x[c | (1 << HI)], x[c | (1 << HI) | (1 << LO)]};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            amp_t acc = cmul(cplx{m[8 * r], m[8 * r + 1]}, in[0]);
#pragma unroll
            for (int cc = 1; cc < 4; ++cc) acc = cfma(cplx{m[8 * r + 2 * cc], m[8 * r + 2 * cc + 1]}, in[cc], acc);
            x[c | ((r >> 1) << HI) | ((r & 1) << LO)] = acc;
        }
    }
}

__device__ __forceinline__ void seq_run(amp_t (&x)[32], const SeqGate *__restrict__ gates, int n_gates) {
#pragma unroll 1
    for (int g = 0; g < n_gates; ++g) {
        const double *m = gates[g].m;
        switch (gates[g].code) {     // wave-uniform (scalar loads)
            case 0: seq_apply1<0>(x, m); break;
            case 1: seq_apply1<1>(x, m); break;
            case 2: seq_apply1<2>(x, m); break;
            case 3: seq_apply1<3>(x, m); break;
            case 4: seq_apply1<4>(x, m); break;
            case 5: seq_apply2<1, 0>(x, m); break;
            case 6: seq_apply2<2, 0>(x, m); break;
            case 7: seq_apply2<2, 1>(x, m); break;
            case 8: seq_apply2<3, 0>(x, m); break;
            case 9: seq_apply2<3, 1>(x, m); break;
            case 10: seq_apply2<3, 2>(x, m); break;
            case 11: seq_apply2<4, 0>(x, m); break;
            case 12: seq_apply2<4, 1>(x, m); break;
            case 13: seq_apply2<4, 2>(x, m); break;
            default: seq_apply2<4, 3>(x, m); break;
        }
    }
}

// every target on bit 6 or higher: k_dense_big<5, 0>'s loads and in-place stores around the gate sequence
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seq_big(amp_t *__restrict__ a, const BigArgs g, const SeqGate *__restrict__ gates,
                                                      int n_gates, const uint64_t *__restrict__ hoff) {
    constexpr int D = 32;
    const uint64_t tile = (g.regions > 1 && gridDim.x % g.regions == 0)
                              ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                              : blockIdx.x;
    const uint64_t w = g.w0 + tile * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (w >= g.W) return;
    const uint64_t base = deposit(w, g);
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    seq_run(x, gates, n_gates);
#pragma unroll
    for (int c = 0; c < D; ++c) st<NT>(a + base + hoff[c], x[c]);
}

// targets below bit 6: k_dense_lds<5, KB>'s addressing and LDS exchange around the gate sequence
template <int KB, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seq_lds(amp_t *__restrict__ a, const LdsArgs g, const SeqGate *__restrict__ gates,
                                                      int n_gates, const uint64_t *__restrict__ hoff) {
    constexpr int D = 32, NB = 1 << KB;
    __shared__ amp_t tiles[KB > 0 ? NB * QSV_BLOCK : 1];
    amp_t *tile = tiles + (KB > 0 ? NB * 64 * (threadIdx.x >> 6) : 0);
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    const uint64_t w = g.w0 + tile_id * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x;
    if (w >= g.W) return;  // W and w0 are multiples of 64: whole waves leave together
    const uint32_t lane = threadIdx.x & 63;
    uint64_t base = deposit(w, g) & ~static_cast<uint64_t>(g.amask);
    for (int j = 0; j < g.na; ++j) base |= static_cast<uint64_t>((lane >> g.abit[j]) & 1u) << g.aE[j];
    amp_t x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ld<NT>(a + base + hoff[c]);
    uint32_t my_row = 0;
    if constexpr (KB > 0) {
#pragma unroll
        for (int v = 1; v < NB; ++v)
            if ((lane & g.bmask) == g.bdep[v]) my_row = v;
#pragma unroll
        for (int o = 0; o < D / NB; ++o) {
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) tile[s * 64 + (lane ^ g.bdep[s])] = x[o * NB + s];
            wave_sync();
#pragma unroll
            for (int t = 0; t < NB; ++t) x[o * NB + t] = tile[my_row * 64 + (lane ^ g.bdep[t])];
        }
    }
    seq_run(x, gates, n_gates);
    if constexpr (KB > 0) {
#pragma unroll
        for (int o = 0; o < D / NB; ++o) {
            wave_sync();
#pragma unroll
            for (int t = 0; t < NB; ++t) tile[my_row * 64 + (lane ^ g.bdep[t])] = x[o * NB + t];
            wave_sync();
#pragma unroll
            for (int s = 0; s < NB; ++s) st<NT>(a + base + hoff[o * NB + s], tile[s * 64 + (lane ^ g.bdep[s])]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; ++c) st<NT>(a + base + hoff[c], x[c]);
    }
}

// ----------------------------------------------------------------------------------------------------
// 6-qubit dense gates.  2^6 complex FMAs per amplitude are 16 flop/B: above the fp64 ridge of the chip (~10 flop/B),
// so this one kernel of the gate path is bounded by arithmetic, not by HBM, and a 64 x 64 matrix times a (64 x groups)
// panel is a GEMM: it runs on the f64 matrix cores (v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15], D col = lane & 15, row = (lane >> 4) + 4 reg; same peak as the vector pipe, but 64
// VGPRs of inputs per lane instead of 256, so two waves per SIMD overlap loads with arithmetic -- the register-blocked
// vector form ran at 8.5 TFLOP/s, one wave per SIMD, stalled on its 1 KiB matrix rows).
// A wave owns 16 groups (the 16 lowest free index values): lane (li, lk) holds amplitudes 4 s + lk, s = 0..15, of group
// li -- lk runs over the two lowest target bits, so whatever the targets are a wave-instruction touches whole 128-byte
// lines (half lines when bits 0, 1 and 2 are all targets).
// The matrix sits in LDS column-major (real and imaginary planes), a complex product is four real MFMAs, a real
// matrix needs two.  Loads and stores are four 256-byte runs per wave-instruction: whole 128-byte lines.
// ----------------------------------------------------------------------------------------------------

struct Mfma6Args {
    uint64_t W;          // groups = amps / 64
    uint64_t or_mask;    // unused (0); lets deposit() serve this struct too
    int32_t nins;        // 6
    uint32_t pos[8];     // ascending target bits (all >= 4)
};

template <int K, bool NT, bool REALM, bool M3 = false>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, (K == 6 && !REALM) ? 2 : 3))) void k_dense_mfma(
    amp_t *__restrict__ a, const Mfma6Args g, const double *__restrict__ Mcol,  // [plane][col][row]
    const uint64_t *__restrict__ hoff) {
    constexpr int D = 1 << K, SL = D / 4 /* k-slices */, RT = D / 16 /* row tiles */;
    extern __shared__ __attribute__((aligned(16))) char smem6[];
    double *mre = reinterpret_cast<double *>(smem6);
    double *mim = mre + D * D;
    uint64_t *off = reinterpret_cast<uint64_t *>(mre + (REALM ? 1 : 2) * D * D);
    for (int i = threadIdx.x; i < (REALM ? 1 : 2) * D * D; i += QSV_BLOCK) mre[i] = Mcol[i];
    if (threadIdx.x < D) off[threadIdx.x] = hoff[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const uint64_t wave = blockIdx.x * (QSV_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (QSV_BLOCK / 64);
    const uint64_t tiles = g.W / 16;
    if (wave >= tiles) return;
    auto fetch = [&](amp_t (&x)[SL], uint64_t tile) {
        const uint64_t base = deposit(tile * 16 + li, g);
#pragma unroll
        for (int s = 0; s < SL; ++s) x[s] = ld<NT>(a + base + off[4 * s + lk]);
    };
    // complex matrices in three real MFMAs per (slice, row tile) instead of four (see row_product_3m; As = Ar + Ai and
    // xs = xr + xi are one VALU add each, next to 64-cycle MFMAs): S1 += Ar xr, S2 += Ai xi, S3 += As xs.  The row tiles
    // are taken in two halves so that the 3 x RT / 2 accumulators stay at 48 registers.
    auto apply3 = [&](const amp_t (&x)[SL], uint64_t tile) {
        constexpr int HT = RT / 2;
        const uint64_t base = deposit(tile * 16 + li, g);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {   // not unrolled: interleaved halves need the registers of both
            f64x4 s1[HT], s2[HT], s3[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) s1[t] = s2[t] = s3[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                double are[HT], aim[HT], asum[HT];
                const double xsum = x[s].x + x[s].y;   // once per half: cheaper than 32 registers held across the tile
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    are[t] = mre[(4 * s + lk) * D + 16 * (h * HT + t) + li];
                    aim[t] = mim[(4 * s + lk) * D + 16 * (h * HT + t) + li];
                    asum[t] = are[t] + aim[t];
                }
#pragma unroll
                for (int t = 0; t < HT; ++t) s1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[t], x[s].x, s1[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < HT; ++t) s2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[t], x[s].y, s2[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < HT; ++t) s3[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(asum[t], xsum, s3[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // in place: the wave's loads of this tile are complete (their values are MFMA operands above) before the
            // first store issues; the second half reads only registers
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    st<NT>(a + base + off[16 * (h * HT + t) + lk + 4 * r],
                           amp_t{s1[t][r] - s2[t][r], s3[t][r] - s1[t][r] - s2[t][r]});
        }
    };
    auto apply4 = [&](const amp_t (&x)[SL], uint64_t tile) {
        f64x4 cre[RT], cim[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) cre[t] = cim[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            double are[RT], aim[RT];
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                are[t] = mre[(4 * s + lk) * D + 16 * t + li];
                if constexpr (!REALM) aim[t] = mim[(4 * s + lk) * D + 16 * t + li];
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {  // dependent updates of one accumulator stay 2 RT instructions apart
                cre[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[t], x[s].x, cre[t], 0, 0, 0);
                cim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[t], x[s].y, cim[t], 0, 0, 0);
            }
            if constexpr (!REALM) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    cre[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim[t], x[s].y, cre[t], 0, 0, 0);
                    cim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[t], x[s].x, cim[t], 0, 0, 0);
                }
            }
            // keep the matrix reads of slice s + 1 behind the MFMAs of slice s: hoisted to the top (the scheduler's
            // choice without this fence) the slices' operands need up to 256 VGPRs and spill
            __builtin_amdgcn_sched_barrier(0);
        }
        // in place: the wave has read every amplitude of its 16 groups before the first of these stores can issue
        const uint64_t base = deposit(tile * 16 + li, g);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                st<NT>(a + base + off[16 * t + lk + 4 * r], amp_t{cre[t][r], cim[t][r]});
    };
    auto apply = [&](const amp_t (&x)[SL], uint64_t tile) {
        if constexpr (M3) apply3(x, tile);
        else apply4(x, tile);
    };
    // A ring of input buffers, no copies between them: the next tiles' loads are in flight while this tile's MFMAs run
    // (K = 6: 256 MFMAs = 7 us per tile, one tile ahead; K = 5: 64 MFMAs = 1.7 us, two ahead).  Every fetch is
    // unconditional -- past the end a wave re-reads its first tile and drops it -- because the compiler cannot count
    // loads issued under a branch and would wait for all of them (see k_rdm).
    // (a real 64 x 64 matrix halves the MFMAs: that variant is bound by memory and runs three waves per SIMD without a
    // ring -- 1.74-2.04 ms by placement, the same as two waves with one (1.74-2.01), in 156 instead of 230 registers)
    constexpr int NBUF = K == 6 ? (REALM ? 1 : 2) : 3;
    amp_t x[NBUF][SL];
    if constexpr (NBUF == 1) {
        for (uint64_t tile = wave; tile < tiles; tile += waves) {
            fetch(x[0], tile);
            apply(x[0], tile);
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b) {
        const uint64_t t = wave + b * waves;
        fetch(x[b], t < tiles ? t : wave);
    }
    for (uint64_t tile = wave; tile < tiles;) {
#pragma unroll
        for (int b = 0; b < NBUF; ++b) {
            const uint64_t t = tile + (NBUF - 1) * waves;
            fetch(x[(b + NBUF - 1) % NBUF], t < tiles ? t : wave);
            apply(x[b], tile);
            tile += waves;
            if (tile >= tiles) break;
        }
    }
}

// Register-to-register copy (qsv_copy; also the "what does a plain copy reach on this box" leg of bench.py), every
// wave-instruction a whole 1 KiB segment, nontemporal both ways (hipMemcpy D2D: 4.9 TB/s).  Forms (QSV_COPY_MODE, for
// measurements; profiles/r03_copy_kernel.txt): 0 = four amplitudes per thread through registers, 1 = one amplitude per
// thread through registers, 2 = one per thread, HBM -> LDS directly (global_load_lds_dwordx4, as the gate kernels
// load) and LDS -> HBM.
constexpr int COPY_ITEMS = 4;
template <int MODE>
__global__ __launch_bounds__(QSV_BLOCK) void k_copy(amp_t *__restrict__ dst, const amp_t *__restrict__ src, uint32_t regions) {
    const uint64_t tile = (regions > 1 && gridDim.x % regions == 0)
                              ? (blockIdx.x % regions) * static_cast<uint64_t>(gridDim.x / regions) + blockIdx.x / regions
                              : blockIdx.x;
    if constexpr (MODE == 0) {
        const uint64_t base = tile * (QSV_BLOCK * COPY_ITEMS) + threadIdx.x;
        amp_t v[COPY_ITEMS];
#pragma unroll
        for (int u = 0; u < COPY_ITEMS; ++u) v[u] = __builtin_nontemporal_load(src + base + u * QSV_BLOCK);
#pragma unroll
        for (int u = 0; u < COPY_ITEMS; ++u) __builtin_nontemporal_store(v[u], dst + base + u * QSV_BLOCK);
    } else if constexpr (MODE == 1) {
        const uint64_t i = tile * QSV_BLOCK + threadIdx.x;
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
    } else {
        __shared__ amp_t lds[QSV_BLOCK];
        const uint64_t i = tile * QSV_BLOCK + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
        __builtin_amdgcn_global_load_lds(src + i, lds + (threadIdx.x & ~63u), 16, 0, 2);
#endif
        __syncthreads();
        __builtin_nontemporal_store(lds[threadIdx.x], dst + i);
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
template <int KH, int KL, int U>
void launch_dense_nt(qsv_state *st, const GateArgs &g, int grid) {
    const bool sub = g.nins > KH || g.lane_ctrl != 0;
    const dim3 gd(grid), bd(QSV_BLOCK);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense%s<%d, %d, %d, %s>", sub ? "_ctrl" : "", KH, KL, U,
             st->nontemporal ? "true" : "false");
    if (st->nontemporal) {
        if (sub) hipLaunchKernelGGL((k_dense_ctrl<KH, KL, U, true>), gd, bd, 0, st->stream, st->data, g);
        else hipLaunchKernelGGL((k_dense<KH, KL, U, true>), gd, bd, 0, st->stream, st->data, g);
    } else {
        if (sub) hipLaunchKernelGGL((k_dense_ctrl<KH, KL, U, false>), gd, bd, 0, st->stream, st->data, g);
        else hipLaunchKernelGGL((k_dense<KH, KL, U, false>), gd, bd, 0, st->stream, st->data, g);
    }
}

// Work items in flight per thread, from the MI355X sweeps under profiles/ (n = 28): with nontemporal
// accesses one item per thread streams best (6.0-6.4 TB/s) until the pair stride reaches 16 MiB (bit 20),
// where four items per thread hold 5.8 TB/s and one item drops to 5.4.
template <int KH, int KL>
int default_unroll(const GateArgs &g) {
    if (KH == 0) return KL == 2 ? 2 : 1;
    bool far = false;  // a pair stride of 16 MiB .. 512 MiB (bits 20..25)
    for (int h = 1; h < (1 << KH); h <<= 1) {
        int bit = 0;
        while ((g.hoff[h] >> bit) > 1) ++bit;
        far = far || (bit >= 20 && bit <= 25);
    }
    if (KH == 1 && KL == 1) return 1;   // round 2 re-sweep: one item per thread at every stride (1.35-1.44 against 1.50-1.53 ms on bits 20..25)
    if (KH == 1 && KL == 0 && far) {
        // single far pair stride: only 16 MiB (bit 20) wants four items per thread (profiles/r01_sweep_far_bits.txt)
        int bit = 0;
        while ((g.hoff[1] >> bit) > 1) ++bit;
        return bit == 20 ? 4 : 1;
    }
    return far ? 4 : 1;
}

template <int KH, int KL>
int launch_dense(qsv_state *st, const GateArgs &g) {
    int U = st->unroll > 0 ? st->unroll : default_unroll<KH, KL>(g);
    // never more unrolling than there is work for one tile
    while (U > 1 && g.W < static_cast<uint64_t>(QSV_BLOCK) * U) U >>= 1;
    GateArgs ga = g;
    ga.ubit = st->ubit;
    // measured on MI355X at n = 28 (profiles/r01_sweep_tile_order.txt): natural-order kernels like 32 regions,
    // pair kernels 8 (one per XCD), except at pair strides of 16..512 MiB where the plain order is best
    if (st->remap >= 0) {
        ga.remap = st->remap;
    } else {
        bool far = false;
        int top = 0;
        for (int h = 1; h < (1 << KH); h <<= 1) {
            int bit = 0;
            while ((g.hoff[h] >> bit) > 1) ++bit;
            far = far || (bit >= 20 && bit <= 25);
            top = bit > top ? bit : top;
        }
        const bool sub = g.nins > KH || g.lane_ctrl != 0;  // controlled / pair-exchange launches: plain order
        if (sub) ga.remap = 0;
        else if (KH == 0) ga.remap = KL == 2 ? 0 : 32;   // round 2 re-sweep (tools/probe_low_pairs.py): 1.35 against 1.41 ms
        else if (KH == 1 && KL == 0) ga.remap = top == 20 ? 0 : top == 24 ? 2 : 8;  // per-stride winners of the sweeps
        else if (KH == 1) ga.remap = (top == 20 || top == 24) ? 32 : 8;   // KL = 1; round 2 re-sweep (tools/probe_retune.py)
        else ga.remap = top < 20 ? 8 : 0;
    }
    while (ga.ubit > 8 && (g.W >> ga.ubit) < static_cast<uint64_t>(U)) --ga.ubit;  // small registers
    const int grid = grid_for(g.W, QSV_BLOCK * U, st->grid_cap);
    switch (U) {
        case 1: launch_dense_nt<KH, KL, 1>(st, ga, grid); break;
        case 2: launch_dense_nt<KH, KL, 2>(st, ga, grid); break;
        case 4: launch_dense_nt<KH, KL, 4>(st, ga, grid); break;
        default: launch_dense_nt<KH, KL, 8>(st, ga, grid); break;
    }
    return check_launch();
}

int launch_diag(qsv_state *st, const DiagArgs &g0) {
    DiagArgs g = g0;
    // full traffic: one item per thread, 32 regions; sub-space launches (Z, CZ, multi-controlled phases):
    // four items per thread, one region per XCD (profiles/r01_sweep_sub_kernels.txt)
    const bool sub = g0.nins > 0 || g0.lane_ctrl != 0;
    g.remap = st->remap >= 0 ? st->remap : (sub ? 8 : 32);
    int U = st->unroll > 0 ? st->unroll : (sub ? 4 : 1);
    while (U > 1 && g.W < static_cast<uint64_t>(QSV_BLOCK) * U) U >>= 1;
    const dim3 gd(grid_for(g.W, QSV_BLOCK * U, st->grid_cap)), bd(QSV_BLOCK);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag<%d, %s>%s", U, st->nontemporal ? "true" : "false",
             (g.nins > 0 || g.lane_ctrl) ? " [sub-space]" : "");
#define QSV_LAUNCH_DIAG(UU)                                                                  \
    if (st->nontemporal)                                                                      \
        hipLaunchKernelGGL((k_diag<UU, true>), gd, bd, 0, st->stream, st->data, g);            \
    else                                                                                      \
        hipLaunchKernelGGL((k_diag<UU, false>), gd, bd, 0, st->stream, st->data, g)
    switch (U) {
        case 1: QSV_LAUNCH_DIAG(1); break;
        case 2: QSV_LAUNCH_DIAG(2); break;
        case 4: QSV_LAUNCH_DIAG(4); break;
        default: QSV_LAUNCH_DIAG(8); break;
    }
#undef QSV_LAUNCH_DIAG
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

// ----------------------------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------------------------
int qsvk_ensure_matrix(qsv_state *st, size_t bytes) {
    if (st->dev_matrix_bytes >= bytes) return QSV_OK;
    if (st->dev_matrix) {
        QSV_HIP(hipStreamSynchronize(st->stream));
        QSV_HIP(hipFree(st->dev_matrix));
        st->dev_matrix = nullptr;
        st->dev_matrix_bytes = 0;
    }
    if (hipMalloc(reinterpret_cast<void **>(&st->dev_matrix), bytes) != hipSuccess)
        return qsv_fail(QSV_ENOMEM, "device allocation of the gate-matrix buffer failed");
    st->dev_matrix_bytes = bytes;
    return QSV_OK;
}

// Gate matrices and index tables come from host memory that dies when the call returns.  Copying them to the device
// with hipMemcpyAsync + hipStreamSynchronize makes every such gate wait for the previous kernel before its own launch
// can even be queued: 72 us of idle GPU between the fused blocks of a circuit (4 % of the pass at n = 28, two thirds of
// it at n = 22).  Instead the data is copied into the next slot of a pinned ring by the CPU, a transfer to the slot's
// device mirror is queued on the register's stream in front of the kernel, and an event recorded behind the
// kernel says when the slot may be overwritten -- the host only ever waits when it is a whole ring ahead of the GPU.
// Payloads larger than a slot take the synchronous road through st->dev_matrix.
// The transfer itself is a small kernel that reads the pinned slot over PCIe (pinned host memory is mapped into the
// device's address space): a copy-engine transfer queued between two kernels starts ~45 us after the first kernel ends
// (the dependency crosses from the compute queue to the SDMA queue), a kernel behind a kernel on the same queue ~5 us.
__global__ __launch_bounds__(QSV_BLOCK) void k_stage_copy(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint32_t n16) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

int qsvk_stage(qsv_state *st, const void *a, size_t bytes_a, const void *b, size_t bytes_b, StageRef *out) {
    const size_t off_b = qsv_pad16(bytes_a), total = off_b + bytes_b;
    if (total > QSV_STAGE_BYTES) {
        const int rc = qsvk_ensure_matrix(st, total);
        if (rc) return rc;
        char *dev = reinterpret_cast<char *>(st->dev_matrix);
        if (bytes_a) QSV_HIP(hipMemcpyAsync(dev, a, bytes_a, hipMemcpyHostToDevice, st->stream));
        if (bytes_b) QSV_HIP(hipMemcpyAsync(dev + off_b, b, bytes_b, hipMemcpyHostToDevice, st->stream));
        QSV_HIP(hipStreamSynchronize(st->stream));  // the sources are pageable host memory that dies at return
        out->dev = dev;
        out->slot = -1;
        return QSV_OK;
    }
    if (!st->stage_dev) {
        // events first, then the buffers; stage_dev is published last, so a failure half way leaves the ring absent
        // (not half built) and the next call starts over
        hipEvent_t events[QSV_STAGE_SLOTS] = {};
        for (int i = 0; i < QSV_STAGE_SLOTS; ++i)
            if (hipEventCreate(&events[i]) != hipSuccess) {
                for (int j = 0; j < i; ++j) (void)hipEventDestroy(events[j]);
                return qsv_fail(QSV_EHIP, "event creation for the gate-matrix staging ring failed");
            }
        char *host = nullptr, *dev = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&host), QSV_STAGE_SLOTS * QSV_STAGE_BYTES, 0) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&dev), QSV_STAGE_SLOTS * QSV_STAGE_BYTES) != hipSuccess) {
            if (host) (void)hipHostFree(host);
            for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
            return qsv_fail(QSV_ENOMEM, "allocation of the gate-matrix staging ring failed");
        }
        for (int i = 0; i < QSV_STAGE_SLOTS; ++i) st->stage_done[i] = events[i];
        st->stage_host = host;
        st->stage_dev = dev;
    }
    const int slot = static_cast<int>(st->stage_next++ % QSV_STAGE_SLOTS);
    if (st->stage_busy[slot]) {
        QSV_HIP(hipEventSynchronize(st->stage_done[slot]));
        st->stage_busy[slot] = false;
    }
    char *host = st->stage_host + slot * QSV_STAGE_BYTES, *dev = st->stage_dev + slot * QSV_STAGE_BYTES;
    if (bytes_a) std::memcpy(host, a, bytes_a);
    if (bytes_b) std::memcpy(host + off_b, b, bytes_b);
    const uint32_t n16 = static_cast<uint32_t>((total + 15) / 16);
    hipLaunchKernelGGL(k_stage_copy, dim3((n16 + QSV_BLOCK - 1) / QSV_BLOCK < 16 ? (n16 + QSV_BLOCK - 1) / QSV_BLOCK : 16), dim3(QSV_BLOCK), 0,
                       st->stream, reinterpret_cast<uint4 *>(dev), reinterpret_cast<const uint4 *>(host), n16);
    QSV_HIP(hipGetLastError());
    // the slot is protected from here on: whatever the caller does next (its launch may fail, it may return early), the
    // pinned slot is not rewritten before this copy kernel has read it.  qsvk_stage_done moves the mark behind the consumer.
    QSV_HIP(hipEventRecord(st->stage_done[slot], st->stream));
    st->stage_busy[slot] = true;
    out->dev = dev;
    out->slot = slot;
    return QSV_OK;
}

int qsvk_stage_done(qsv_state *st, const StageRef &ref) {
    if (ref.slot < 0) return QSV_OK;
    QSV_HIP(hipEventRecord(st->stage_done[ref.slot], st->stream));   // re-record: now behind the kernel that reads the slot
    st->stage_busy[ref.slot] = true;
    return QSV_OK;
}

// Out-of-place operations (measure, insert, permute, the mode contractions) write into the state's spare
// buffer and then swap it in (qsvk_adopt).  The spare is kept between calls: a circuit that alternates such
// operations ping-pongs between two allocations instead of paying hipMalloc/hipFree of the register per gate
// (measured: ~0.44 s per gate on a 16 GiB register).
int qsvk_scratch(qsv_state *st, uint64_t amps, amp_t **out) {
    if (amps == 0) amps = 1;
    if (st->spare_capacity < amps) {
        if (st->spare) {
            QSV_HIP(hipStreamSynchronize(st->stream));
            QSV_HIP(hipFree(st->spare));
            st->spare = nullptr;
            st->spare_capacity = 0;
        }
        if (hipMalloc(reinterpret_cast<void **>(&st->spare), sizeof(amp_t) * amps) != hipSuccess)
            return qsv_fail(QSV_ENOMEM, "device allocation of the spare register failed");
        st->spare_capacity = amps;
    }
    *out = st->spare;
    return QSV_OK;
}

// The spare buffer now holds the register (new_amps amplitudes): swap it in when the library owns the memory,
// copy it back when the caller does (a view's pointer must stay valid).
int qsvk_adopt(qsv_state *st, uint64_t new_amps) {
    if (st->owns_data) {
        std::swap(st->data, st->spare);
        std::swap(st->capacity, st->spare_capacity);
    } else {
        QSV_HIP(hipMemcpyAsync(st->data, st->spare, sizeof(amp_t) * new_amps, hipMemcpyDeviceToDevice, st->stream));
    }
    st->amps = new_amps;
    return QSV_OK;
}


// The dispatches of one launch of g.W work items, at most `limit` each: launch(count) with g.w0 set to the range's start.
template <class Args, class Launch>
static int launch_ranges(Args &g, uint64_t limit, Launch &&launch) {
    for (const Range &r : dispatch_ranges(g.W, limit)) {
        g.w0 = r.w0;
        launch(r.count);
        const int rc = check_launch();
        if (rc) return rc;
    }
    return QSV_OK;
}

static uint32_t regions_or(const qsv_state *st, uint32_t by_default) {   // QSV_OPT_REMAP overrides a form's tile order
    return st->remap >= 0 ? static_cast<uint32_t>(st->remap) : by_default;
}

// ---- k-qubit dense gate, targets on bits >= 3, staged through LDS: "tile" form -------------------------------------
// k_dense_big gives every thread a whole 2^K-amplitude column (128 VGPRs at K = 5: two or three waves per SIMD that
// load, compute and store in lock step).  Here a workgroup of 2^K / ROWS waves owns 64 columns: wave q loads inputs
// q ROWS .. q ROWS + ROWS - 1 of every column (1 KiB per wave-instruction: the 64 columns are the 64 lowest free index
// values, so lanes 8j..8j+7 cover one whole 128-byte line whatever the target bits >= 3 are), parks them in a
// [2^K][64] LDS tile, and after one barrier computes outputs q ROWS .. q ROWS + ROWS - 1 of its lane's column: the 2^K
// inputs come back from LDS one 16-byte read each (lane-contiguous, conflict-free), the ROWS x 2^K slice of the matrix
// is wave-uniform and arrives as SGPR operands.  ROWS accumulators instead of 2^K amplitudes per thread: five
// workgroups per CU (LDS-bound at K = 5), whose load / compute / store phases overlap.
template <int K, int ROWS, bool REAL, bool NT, bool M3 = false>
__global__ __launch_bounds__((1 << K) / ROWS * 64) void k_dense_tile(amp_t *__restrict__ a, const BigArgs g,
                                                                     const double *__restrict__ mat,   // [q][c][ROWS]
                                                                     const uint64_t *__restrict__ off) {
    static_assert(!(REAL && M3), "a real matrix needs two multiplications per entry anyway");
    constexpr int PER = REAL ? 1 : M3 ? 3 : 2;   // doubles per matrix entry: re | (re, im) | (re, im, re + im)
    constexpr int D = 1 << K;
    __shared__ amp_t tile[D * 64];
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile order as in k_dense: `regions` contiguous pieces of this launch's range walked side by side
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    const uint64_t base = deposit(g.w0 + tile_id * 64 + lane, g);
    uint64_t o[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) o[i] = off[q * ROWS + i];
    // HBM -> LDS without a stop in the registers (global_load_lds_dwordx4: lane l of the wave lands at the row's base + 16 l)
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
        __builtin_amdgcn_global_load_lds(a + base + o[i], tile + (q * ROWS + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    __syncthreads();
    amp_t acc[ROWS];
    double s3[M3 ? ROWS : 1];   // 3M form (see row_product_3m): acc.x = sum Ar xr, acc.y = sum Ai xi, s3 = sum As xs
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i] = amp_t{0.0, 0.0};
    if constexpr (M3) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) s3[i] = 0.0;
    }
    const double *m = mat + static_cast<size_t>(q) * D * ROWS * PER;
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const amp_t v = tile[c * 64 + lane];
        const double *mc = m + c * ROWS * PER;
        [[maybe_unused]] const double vs = v.x + v.y;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            if constexpr (REAL) {
                acc[i].x = fma(mc[i], v.x, acc[i].x);
                acc[i].y = fma(mc[i], v.y, acc[i].y);
            } else if constexpr (M3) {
                acc[i].x = fma(mc[3 * i], v.x, acc[i].x);
                acc[i].y = fma(mc[3 * i + 1], v.y, acc[i].y);
                s3[i] = fma(mc[3 * i + 2], vs, s3[i]);
            } else {
                acc[i] = cfma(cplx{mc[2 * i], mc[2 * i + 1]}, v, acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        amp_t out = acc[i];
        if constexpr (M3) out = amp_t{acc[i].x - acc[i].y, s3[i] - acc[i].x - acc[i].y};
        if (NT) __builtin_nontemporal_store(out, a + base + o[i]);
        else a[base + o[i]] = out;
    }
}

// ---- a fused block as the SEQUENCE of its source gates on an LDS-resident tile (round 3) -------------------------------
// Dense 5- and 6-qubit blocks are the gate shapes bound by arithmetic (4 x 32 / 3 x 64 real multiply-adds per amplitude at
// a power-limited clock: 1.6 / 1.9 ms against the 1.31 ms of a pass over HBM), yet a fused block is the product of a
// handful of 1- and 2-qubit gates worth 4-8 multiply-adds each.  Here a workgroup brings a 4096-amplitude tile into LDS
// -- the block's K target bits plus the 12 - K lowest other bits: every row of the tile is 64 contiguous amplitudes (bits
// 0-5 are always in the tile when K <= 6), so HBM sees whole 1 KiB runs in both directions, straight into LDS on the way
// in -- and applies the source gates one after the other on that 12-qubit register (a barrier between gates), as the
// single-launch executor does with whole registers (qsv_circuit.hip).  Two workgroups per CU: one computes while the
// other loads or stores.
// The gate list is cut into PASSES over at most four tile bits each (consecutive gates whose legs fit four bits together):
// a thread takes the 16 amplitudes of one group of the pass's four bits into registers, applies the pass's gates there
// (seq_apply*: compile-time register indices behind a wave-uniform switch) and puts them back -- one LDS round trip and one
// barrier per pass instead of one per gate.

constexpr int TILE_SEQ_ROWS_PER_WAVE = TILE_SEQ_ROWS / (TILE_SEQ_THREADS / 64);

struct TileSeqArgs {
    BigArgs g;              // pos[] = ALL tile bits: the tile number is deposited around them
    uint32_t lane_bit[6];   // address bit of lane bit j (the six lowest tile bits: 0..5 unless a 6-qubit block sits above them)
};

__device__ __forceinline__ void seq_run16(amp_t (&x)[16], const SeqGate *__restrict__ gates, int n_gates) {
#pragma unroll 1
    for (int g = 0; g < n_gates; ++g) {
        const double *m = gates[g].m;
        switch (gates[g].code) {     // wave-uniform (scalar loads): 0..3 one-qubit gates, 5 + p two-qubit gates as in SeqGate
            case 0: seq_apply1<0, 16>(x, m); break;
            case 1: seq_apply1<1, 16>(x, m); break;
            case 2: seq_apply1<2, 16>(x, m); break;
            case 3: seq_apply1<3, 16>(x, m); break;
            case 5: seq_apply2<1, 0, 16>(x, m); break;
            case 6: seq_apply2<2, 0, 16>(x, m); break;
            case 7: seq_apply2<2, 1, 16>(x, m); break;
            case 8: seq_apply2<3, 0, 16>(x, m); break;
            case 9: seq_apply2<3, 1, 16>(x, m); break;
            default: seq_apply2<3, 2, 16>(x, m); break;
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(TILE_SEQ_THREADS) void k_seq_tile(amp_t *__restrict__ a, const TileSeqArgs ta,
                                                              const SeqGate *__restrict__ gates,
                                                              const TilePass *__restrict__ passes, int n_passes,
                                                              const uint64_t *__restrict__ off) {   // [rows] row offsets
    const BigArgs &g = ta.g;
    extern __shared__ __attribute__((aligned(16))) char seq_smem[];
    amp_t *tile = reinterpret_cast<amp_t *>(seq_smem);        // [rows][64 lanes] = the tile register, index row * 64 + lane
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave q: rows q RPW .. q RPW + RPW - 1
    constexpr int RPW = TILE_SEQ_ROWS_PER_WAVE;
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    uint64_t base = deposit(g.w0 + tile_id, g);
#pragma unroll
    for (int j = 0; j < 6; ++j) base |= static_cast<uint64_t>((lane >> j) & 1) << ta.lane_bit[j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < RPW; ++i)
        __builtin_amdgcn_global_load_lds(a + base + off[q * RPW + i], tile + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < n_passes; ++p) {
        const TilePass &ps = passes[p];
        // the groups of the pass: their index bits with zeros inserted at the pass's four tile bits
        for (uint32_t grp = threadIdx.x; grp < (1u << (TILE_SEQ_BITS - 4)); grp += TILE_SEQ_THREADS) {
            uint32_t g0 = grp;
#pragma unroll
            for (int j = 0; j < 4; ++j) g0 = static_cast<uint32_t>(insert_zero(g0, ps.q[j]));
            amp_t x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c)
                x[c] = tile[g0 | ((c & 1) << ps.q[0]) | (((c >> 1) & 1) << ps.q[1]) | (((c >> 2) & 1) << ps.q[2]) | (((c >> 3) & 1) << ps.q[3])];
            seq_run16(x, gates + ps.first, ps.count);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                tile[g0 | ((c & 1) << ps.q[0]) | (((c >> 1) & 1) << ps.q[1]) | (((c >> 2) & 1) << ps.q[2]) | (((c >> 3) & 1) << ps.q[3])] = x[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) st<NT>(a + base + off[q * RPW + i], tile[(q * RPW + i) * 64 + lane]);
}

// Complex 5-qubit blocks: the LDS tile of k_dense_tile feeding the f64 MATRIX CORES (round 3).  The vector kernels spend
// 4 x 32 FP64 FMAs per amplitude; rocprofv3's SQ counters put their vector pipe at 81 % busy over the whole launch, at a
// clock that the FP64 load pulls down to ~1.65 GHz (a 1-qubit gate runs at 2.3): they are bound by arithmetic, and the
// three-multiplication form does not help them because its third plane of matrix rows (24 KiB per gate) no longer fits
// the scalar cache the rows stream through.  Here the matrix lives in REGISTERS for the whole launch -- lane (i, kk)
// holds M[16 t + i][4 s + kk] of every (row tile t, slice s): 32 complex values + their sums, 96 registers -- as the A
// operand of v_mfma_f64_16x16x4_f64, and a complex product is three MFMAs (S1 += Ar xr, S2 += Ai xi, S3 += (Ar + Ai)(xr +
// xi)): 48 MFMAs per 16 groups instead of 4096 wave-FMAs.  The HBM side is k_dense_tile's: a workgroup owns 64 columns,
// wave q brings input rows 8 q .. 8 q + 7 straight into the [32][64] LDS tile (1 KiB per wave-instruction), then takes
// the 16 columns 16 q .. 16 q + 15 through the matrix cores (B operand: lane (j, kk) reads [4 s + kk][16 q + j]), puts
// the results back into its own columns of the tile, and after a barrier stores rows 8 q .. again as whole 1 KiB runs.
// Persistent workgroups (the matrix registers are loaded once).
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_dense_mtile5(
    amp_t *__restrict__ a, const BigArgs g, const double *__restrict__ mat /* [r][c] (re, im) */,
    const uint64_t *__restrict__ off) {
    constexpr int D = 32, ROWS = 8;
    __shared__ amp_t tiles[2][D * 64];   // two tiles: the next one is on its way from HBM while this one is computed and stored
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double are[8][2], aim[8][2], asum[8][2];
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const double *e = mat + 2 * ((16 * t + li) * D + 4 * s + lk);
            are[s][t] = e[0];
            aim[s][t] = e[1];
            asum[s][t] = e[0] + e[1];
        }
    uint64_t o[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) o[i] = off[q * ROWS + i];
    const uint64_t n_tiles = g.W / 64;
    auto base_of = [&](uint64_t t0) {
        const uint64_t tile_id = (g.regions > 1 && n_tiles % g.regions == 0) ? (t0 % g.regions) * (n_tiles / g.regions) + t0 / g.regions : t0;
        return deposit(g.w0 + tile_id * 64 + lane, g);
    };
    auto fetch = [&](uint64_t base, amp_t *tile) {
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
            __builtin_amdgcn_global_load_lds(a + base + o[i], tile + (q * ROWS + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    };
    // Barriers are raw s_barrier + counted waits: __syncthreads() carries a fence that drains the vector-memory counter, i.e.
    // waits for the NEXT tile's loads (issued just before) and for this tile's stores.  The counter retires loads, stores and
    // LDS-DMA in issue order, so at the top of an iteration "all but the 8 youngest" = the previous tile's 8 stores may stay
    // in flight while this tile's 8 loads (older) are complete.
    uint64_t t0 = blockIdx.x;
    uint64_t base = base_of(t0);
    fetch(base, tiles[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int it = 0; t0 < n_tiles; t0 += gridDim.x, ++it) {
        amp_t *tile = tiles[it & 1];
        // this tile's loads have landed (every wave waits for its own, then the barrier), and nobody reads the other tile
        // any more (the LDS reads of the previous store phase have returned)
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const uint64_t next = t0 + gridDim.x;
        const uint64_t next_base = base_of(next < n_tiles ? next : blockIdx.x);   // past the end: re-read the first tile, unused
        fetch(next_base, tiles[(it & 1) ^ 1]);
        f64x4 s1[2], s2[2], s3[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) s1[t] = s2[t] = s3[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const amp_t x = tile[(4 * s + lk) * 64 + 16 * q + li];
            const double xs = x.x + x.y;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[s][t], x.x, s1[t], 0, 0, 0);
                s2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[s][t], x.y, s2[t], 0, 0, 0);
                s3[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(asum[s][t], xs, s3[t], 0, 0, 0);
            }
        }
        // this wave has read everything it needs from its 16 columns (the reads are MFMA operands above): results in place
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tile[(16 * t + lk + 4 * r) * 64 + 16 * q + li] = amp_t{s1[t][r] - s2[t][r], s3[t][r] - s1[t][r] - s2[t][r]};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my results are in the tile; the next tile's loads stay in flight
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const amp_t v = tile[(q * ROWS + i) * 64 + lane];
            if (NT) __builtin_nontemporal_store(v, a + base + o[i]);
            else a[base + o[i]] = v;
        }
        base = next_base;
    }
}

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

static bool mtile_default() {
    static const bool on = [] { const char *e = getenv("QSV_MTILE"); return e ? atoi(e) != 0 : false; }();
    return on;
}

// k = 3..6 in the form f (choose_form: FORM_MTILE5, FORM_TILE, FORM_LDS or FORM_BIG).  bits[j] = bit position of matrix
// leg j (leg 0 most significant).
static int launch_dense_big(qsv_state *st, int k, const int *bits, const double *m_user, const FormChoice &f) {
    const int D = 1 << k;
    const bool tile = f.form == FORM_TILE, lds = f.form == FORM_LDS;
    // register index c = (h << KL) | t: h bit i <-> high[i], t bit j <-> low[j] (stored at stand-in bit standin[j])
    const Split s = f.transposed ? split_targets(k, bits, st->n) : untransposed(k, bits);
    const int KL = static_cast<int>(s.low.size()), KB = s.KB;
    const std::vector<uint64_t> off = offsets(address_bits(s, lds));
    const std::vector<int> ui = user_index(k, bits, kernel_bits(s).data()), ins = inserted_bits(s);
    // k_dense_tile: the matrix slice of wave q, input c, is ROWS consecutive entries  [q][c][i] = m[q ROWS + i][c]
    const int rows = !tile ? 0 : k == 5 ? 8 : k == 4 ? 4 : 2;
    const std::vector<double> m = matrix(f.realm ? MAT_REAL : !f.m3 ? MAT_COMPLEX : tile ? MAT_3M_ENTRIES : MAT_3M_ROWS, D, m_user,
                                         ui.data(), rows);
    // matrix and offsets ride the staging ring to the device: queued on the stream in front of the kernel, no host wait
    StageRef staged;
    int rc = qsvk_stage(st, m.data(), sizeof(double) * m.size(), off.data(), sizeof(uint64_t) * D, &staged);
    if (rc) return rc;
    const double *dev_m = reinterpret_cast<const double *>(staged.dev);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(sizeof(double) * m.size()));
    const Enumeration e = enumeration(st->amps >> k, ins);
    bool nt = st->nontemporal != 0;  // tile and line-granular forms: every wave-instruction touches whole 128-byte lines
    if (f.form == FORM_MTILE5) {
        BigArgs g = with_enumeration<BigArgs>(e);
        g.regions = regions_or(st, tile_regions(k, ins));
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_mtile5<%s>", nt ? "true" : "false");
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, st->device);  // 256 if the query fails
        const dim3 gd(static_cast<unsigned>(std::min<uint64_t>(e.W / 64, 2ull * cus))), bd(QSV_BLOCK);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_dense_mtile5<NT.value>, gd, bd, 0, st->stream, st->data, g, dev_m, dev_off); });
        rc = check_launch();
    } else if (tile) {
        BigArgs g = with_enumeration<BigArgs>(e);
        g.regions = regions_or(st, tile_regions(k, ins));
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_tile<%d, %d, %s, %s%s>", k, rows, f.realm ? "true" : "false",
                 nt ? "true" : "false", f.m3 ? ", true" : "");
        rc = launch_ranges(g, DISPATCH_TILES * 64, [&](uint64_t columns) {
            const dim3 gd(static_cast<unsigned>(columns / 64));
            with_int<3, 5>(k, [&](auto K) { with_bool(f.realm, [&](auto REAL) { with_bool(nt, [&](auto NT) {
                constexpr int ROWS = K.value == 5 ? 8 : K.value == 4 ? 4 : 2;
                const dim3 bd((1 << K.value) / ROWS * 64);
                if constexpr (K.value == 5 && !REAL.value) {
                    if (f.m3) {
                        hipLaunchKernelGGL((k_dense_tile<5, ROWS, false, NT.value, true>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_dense_tile<K.value, ROWS, REAL.value, NT.value>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
            }); }); });
        });
    } else if (lds) {
        LdsArgs g = with_enumeration<LdsArgs>(e);
        set_low_fields(g, low_fields(s));
        g.regions = regions_or(st, 8);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_lds<%d, %d, %s, %s%s>", k, KB, nt ? "true" : "false",
                 f.realm ? "true" : "false", f.m3 ? ", 256, true" : "");
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_int<3, 6>(k, [&](auto K) { with_int<0, 3>(KB, [&](auto B) { with_bool(f.realm, [&](auto REAL) { with_bool(nt, [&](auto NT) {
                if constexpr (K.value == 5 && !REAL.value) {
                    if (f.m3) {
                        hipLaunchKernelGGL((k_dense_lds<5, B.value, NT.value, false, QSV_BLOCK, true>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_dense_lds<K.value, B.value, NT.value, REAL.value, QSV_BLOCK>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
            }); }); }); });
        });
    } else {
        BigArgs g = with_enumeration<BigArgs>(e);
        for (int j = 0; j < KL; ++j) g.lbit[j] = s.low[j];
        // partial-line nontemporal accesses are slow: use them only when every access is a full 1 KiB per wave
        bool coalesced = true;
        for (int b : ins) coalesced = coalesced && b >= QSV_LANE_BITS;
        nt = nt && coalesced;
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_big<%d, %d, %s%s>", k, KL, nt ? "true" : "false", f.m3 ? ", true" : "");
        g.regions = regions_or(st, 8);
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_int<3, 5>(k, [&](auto K) { with_int<0, K.value>(KL, [&](auto T) { with_bool(nt, [&](auto NT) {
                if constexpr (K.value == 5 && T.value == 0) {
                    if (f.m3) {
                        hipLaunchKernelGGL((k_dense_big<5, 0, NT.value, true>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_dense_big<K.value, T.value, NT.value>), gd, bd, 0, st->stream, st->data, g, dev_m, dev_off);
            }); }); });
        });
    }
    return rc ? rc : qsvk_stage_done(st, staged);
}


// A fused 5-qubit block as the sequence of its source gates (k_seq_big / k_seq_lds).  bits[j] = bit position of block leg j;
// gate g acts on block legs legs[2 g] (and legs[2 g + 1] when arity[g] == 2), its matrix follows the previous gate's in
// `mats` (8 or 32 doubles).  QSV_UNHANDLED_KQ: the register or the sequence does not fit this form (the caller applies
// the block's product matrix instead).
int qsvk_sequence5(qsv_state *st, const int *bits, int n_gates, const int *arity, const int *legs, const double *mats) {
    const int k = 5, D = 32;
    if (n_gates < 1 || n_gates > SEQ_MAX_GATES || st->n < k) return QSV_UNHANDLED_KQ;
    // multiply-adds per 32 amplitudes: 256 per one-qubit gate, 512 per two-qubit gate, 4096 for the dense block
    int work = 0;
    for (int gi = 0; gi < n_gates; ++gi) work += arity[gi] == 1 ? 256 : 512;
    if (work > (st->sequence_work >= 0 ? st->sequence_work : seq_max_work())) return QSV_UNHANDLED_KQ;
    const uint64_t W = st->amps >> k;
    if (W < 64 || W % 64) return QSV_UNHANDLED_KQ;
    // register index c = (h << KL) | t: h bit i <-> high[i], t bit j <-> low[j] (as launch_dense_big's line-granular form)
    const Split s = split_targets(k, bits, st->n);
    if (!s.enough) return QSV_UNHANDLED_KQ;
    const std::vector<int> kb = kernel_bits(s);
    auto reg_bit = [&](int leg) { return static_cast<int>(std::find(kb.begin(), kb.end(), bits[leg]) - kb.begin()); };
    std::vector<SeqGate> rec(n_gates);
    const double *m = mats;
    for (int gi = 0; gi < n_gates; ++gi) {
        const int l0 = legs[2 * gi], l1 = legs[2 * gi + 1];
        if (arity[gi] == 1) {
            if (l0 < 0 || l0 >= k) return qsv_fail(QSV_EINVAL, "gate sequence: leg outside the block");
            rec[gi] = seq_record(1, reg_bit(l0), 0, m);
        } else if (arity[gi] == 2) {
            if (l0 < 0 || l0 >= k || l1 < 0 || l1 >= k || l0 == l1) return qsv_fail(QSV_EINVAL, "gate sequence: legs outside the block");
            rec[gi] = seq_record(2, reg_bit(l0), reg_bit(l1), m);
        } else {
            return QSV_UNHANDLED_KQ;
        }
        m += arity[gi] == 1 ? 8 : 32;
    }
    const std::vector<uint64_t> off = offsets(address_bits(s, true));
    StageRef staged;
    int rc = qsvk_stage(st, rec.data(), sizeof(SeqGate) * rec.size(), off.data(), sizeof(uint64_t) * D, &staged);
    if (rc) return rc;
    const SeqGate *dev_g = reinterpret_cast<const SeqGate *>(staged.dev);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(sizeof(SeqGate) * rec.size()));
    const bool nt = st->nontemporal != 0;
    const Enumeration e = enumeration(W, inserted_bits(s));
    if (s.low.empty()) {
        BigArgs g = with_enumeration<BigArgs>(e);
        g.regions = regions_or(st, 8);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_big<%s>", nt ? "true" : "false");
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_seq_big<NT.value>, gd, bd, 0, st->stream, st->data, g, dev_g, n_gates, dev_off); });
        });
    } else {
        LdsArgs g = with_enumeration<LdsArgs>(e);
        set_low_fields(g, low_fields(s));
        g.regions = regions_or(st, 8);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_lds<%d, %s>", s.KB, nt ? "true" : "false");
        rc = launch_ranges(g, DISPATCH_ITEMS, [&](uint64_t items) {
            const dim3 gd(grid_for(items, QSV_BLOCK, 0)), bd(QSV_BLOCK);
            with_int<0, 3>(s.KB, [&](auto B) { with_bool(nt, [&](auto NT) {
                hipLaunchKernelGGL((k_seq_lds<B.value, NT.value>), gd, bd, 0, st->stream, st->data, g, dev_g, n_gates, dev_off);
            }); });
        });
    }
    return rc ? rc : qsvk_stage_done(st, staged);
}

// A fused block of k = 1..6 qubits as the list of its source gates on LDS tiles (k_seq_tile).  Arguments as
// qsvk_sequence5.  QSV_UNHANDLED_KQ: the register is too small for a tile, a gate acts on more than two qubits, or the
// list needs more passes than the kernel's table holds.
int qsvk_sequence_tile(qsv_state *st, int k, const int *bits, int n_gates, const int *arity, const int *legs,
                       const double *mats) {
    if (k < 1 || k > 6 || n_gates < 1 || n_gates > SEQ_MAX_GATES || st->n < TILE_SEQ_BITS) return QSV_UNHANDLED_KQ;
    const TileCut cut = cut_tile_passes(st->n, k, bits, n_gates, arity, legs, mats);
    if (cut.status == TileCut::UNHANDLED) return QSV_UNHANDLED_KQ;
    if (cut.status == TileCut::LEG_OUTSIDE) return qsv_fail(QSV_EINVAL, "gate sequence: leg outside the block");
    if (cut.status == TileCut::LEGS_EQUAL) return qsv_fail(QSV_EINVAL, "gate sequence: legs outside the block");
    const std::vector<int> &tile_bits = cut.tile_bits;
    const std::vector<uint64_t> off = offsets(std::vector<int>(tile_bits.begin() + 6, tile_bits.end()));   // [rows]
    // one image: [gates | passes | row offsets]
    const size_t gates_bytes = qsv_pad16(sizeof(SeqGate) * cut.rec.size()), passes_bytes = qsv_pad16(sizeof(TilePass) * cut.passes.size());
    std::vector<char> image(gates_bytes + passes_bytes, 0);
    std::memcpy(image.data(), cut.rec.data(), sizeof(SeqGate) * cut.rec.size());
    std::memcpy(image.data() + gates_bytes, cut.passes.data(), sizeof(TilePass) * cut.passes.size());
    StageRef staged;
    int rc = qsvk_stage(st, image.data(), image.size(), off.data(), sizeof(uint64_t) * off.size(), &staged);
    if (rc) return rc;
    const SeqGate *dev_g = reinterpret_cast<const SeqGate *>(staged.dev);
    const TilePass *dev_p = reinterpret_cast<const TilePass *>(staged.dev + gates_bytes);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(image.size()));
    TileSeqArgs ta;
    std::memset(&ta, 0, sizeof(ta));
    ta.g = with_enumeration<BigArgs>(enumeration(st->amps >> TILE_SEQ_BITS, tile_bits));   // tiles: the index with every tile bit taken out
    for (int j = 0; j < 6; ++j) ta.lane_bit[j] = static_cast<uint32_t>(tile_bits[j]);
    ta.g.regions = regions_or(st, 8);
    const bool nt = st->nontemporal != 0;
    const size_t lds = sizeof(amp_t) << TILE_SEQ_BITS;
    static bool raised = false;
    if (!raised) {
        QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_seq_tile<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)));
        QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_seq_tile<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)));
        raised = true;
    }
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_seq_tile<%s>", nt ? "true" : "false");
    const int n_passes = static_cast<int>(cut.passes.size());
    st->last_passes = n_passes;
    rc = launch_ranges(ta.g, DISPATCH_TILES, [&](uint64_t tiles) {
        const dim3 gd(static_cast<unsigned>(tiles)), bd(TILE_SEQ_THREADS);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_seq_tile<NT.value>, gd, bd, lds, st->stream, st->data, ta, dev_g, dev_p, n_passes, dev_off); });
    });
    return rc ? rc : qsvk_stage_done(st, staged);
}

// ---- deferred gates: one PASS of queued 1- and 2-qubit gates over LDS-resident tiles ----------------------------------
// The queue of a deferring register (qsv_api.hip) is cut into passes by qsv_plan.h.  A workgroup brings one 4096-amplitude
// tile into LDS -- bits 0..5 plus the pass's six further tile bits, so every tile row is one 1 KiB run of HBM, straight
// into LDS on the way in -- applies the pass's gates to it and stores it back: one round trip over HBM for the whole list.
// The gates are applied in GROUPS (qsv_plan::cut_groups: consecutive gates whose targets fit four tile bits): each of the
// 256 threads takes the 16 amplitudes of one setting of the other eight tile bits into registers, applies the group's
// gates there and puts them back -- one LDS round trip and one barrier per group, not per gate (the benchmark circuit: 123 groups for 399 gates in 40 passes;
// measured figures in DESIGN.md section 10).
// Register indices are compile-time: one unrolled body per register bit (1-qubit gates) or ordered pair of them (2-qubit
// gates) and summation form, behind a wave-uniform switch.
// A gate's control bits outside the tile are the same for every amplitude of a tile: they decide per workgroup whether
// the gate acts (omask); a group none of whose gates acts makes no LDS trip, and a tile on which no gate of the pass acts is
// neither loaded nor stored; when some gate of the pass has no outside control (PassArgs::every_tile) the tile is asked for
// first and the controls are looked at under the loads.  A control bit inside the tile is a register bit (rc: amplitudes of
// the thread that the gate skips, wave-uniform) or a thread bit (tc: the new values replace the old ones by a select); the
// bodies exist once per control class (PassGate::ctl), so a gate without controls pays for neither.  Each gate is computed with
// the expression and the summation order of the per-gate kernel it would have run on (tile12_body: products summed from
// zero in kernel-index order; dense_body: low-lane combinations outer, high rows inner; k_diag: one complex product), so
// the amplitudes are bit for bit those of the per-gate path.  A pair exchange moves registers.
constexpr int PASS_TILE = 1 << qsv_plan::TILE_BITS, PASS_ROWS = PASS_TILE / 64, PASS_THREADS = 256;
constexpr int PASS_ROWS_PER_WAVE = PASS_ROWS / (PASS_THREADS / 64);
static_assert(PASS_TILE == PASS_THREADS << qsv_plan::REG_BITS, "one thread per setting of the tile bits outside the registers");

struct PassArgs {
    BigArgs g;                     // pos[] = the 12 tile bits: the tile number is deposited around them, and tile row r
                                   // (tile bits 6..11) starts at the register offset sum_j ((r >> j) & 1) << pos[6 + j]
    uint32_t every_tile;           // some gate of the pass has no control outside the tile: every tile is loaded
};

// Kernel index of the j-th product summed into output row r.  NAT: tile12_body and dense_body without low targets;
// XOR: dense_body with every target a lane bit (x = j over the low combinations); HL: dense_body with one high and one low
// target (x = j >> 1 outer, hp = j & 1 inner, column (hp, l ^ x)).
template <int FORM>
__device__ __forceinline__ constexpr int pass_col(int r, int j) {
    return FORM == 0 ? j : FORM == 1 ? (j ^ r) : (((j & 1) << 1) | ((r & 1) ^ (j >> 1)));
}

// The controls of a gate inside the tile, as one thread sees them.  Every body is compiled once per control class CTL
// (PASS_CTL_*): without controls neither field is read and the new amplitudes are written in place; with controls on
// register bits the register indices b that the gate skips are branched around (wave-uniform); only with controls on
// thread bits do the new values replace the old ones by a select.
struct PassCtl {
    uint32_t rc;     // wave-uniform: register-index bits that must be 1
    bool ok;         // this thread's control bits are all 1
};

template <int CTL>
__device__ __forceinline__ bool pass_skips(int b, const PassCtl &ct) {
    return CTL != PASS_CTL_NONE && (static_cast<uint32_t>(b) & ct.rc) != ct.rc;
}

template <int CTL>
__device__ __forceinline__ void pass_put(amp_t &x, amp_t y, const PassCtl &ct) {
    if constexpr (CTL == PASS_CTL_THREAD) {
        x.x = ct.ok ? y.x : x.x;
        x.y = ct.ok ? y.y : x.y;
    } else {
        x = y;
    }
}

// Dense gate on D amplitudes: kernel index bit 0 <-> register bit P0, bit 1 <-> register bit P1 (D = 4).  Each output is the
// cfma chain from zero over j = 0 .. D - 1 of the per-gate kernels; the chains are written column by column, and in the
// last column every inner product before the first outer one, so that an amplitude has been read for the last time when
// the output that takes its register is produced: the amplitudes are then updated in place, with no second copy of x[].
template <int CTL, int D, int FORM, int P0, int P1>
__device__ __forceinline__ void pass_dense(amp_t (&x)[16], const double *__restrict__ m, const PassCtl &ct) {
    constexpr int TARGETS = (1 << P0) | (D == 4 ? (1 << P1) : 0);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b & TARGETS) continue;
        if (pass_skips<CTL>(b, ct)) continue;      // wave-uniform: a control on a register bit is 0 here
        int idx[D];
#pragma unroll
        for (int c = 0; c < D; ++c) idx[c] = b | ((c & 1) << P0) | (D == 4 ? ((c >> 1) << P1) : 0);
        amp_t acc[D];
#pragma unroll
        for (int r = 0; r < D; ++r) acc[r] = amp_t{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < D - 1; ++j)
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const int c = pass_col<FORM>(r, j);
                acc[r] = cfma(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
            }
        // the last column in cfma's two halves: every inner half before the first outer one
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const int c = pass_col<FORM>(r, D - 1);
            acc[r] = cfma_inner(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
        }
        amp_t y[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const int c = pass_col<FORM>(r, D - 1);
            y[r] = cfma_outer(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < D; ++r) pass_put<CTL>(x[idx[r]], y[r], ct);
    }
}

template <int CTL, int PA, int PB>
__device__ __forceinline__ void pass_pair(amp_t (&x)[16], const PassCtl &ct) {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b & ((1 << PA) | (1 << PB))) continue;
        if (pass_skips<CTL>(b, ct)) continue;
        const amp_t u = x[b | (1 << PA)], v = x[b | (1 << PB)];
        pass_put<CTL>(x[b | (1 << PA)], v, ct);
        pass_put<CTL>(x[b | (1 << PB)], u, ct);
    }
}

// Diagonal gate whose factor for register index c is d[SEL(c)] (d[] per thread or wave-uniform).
template <int CTL, class Sel>
__device__ __forceinline__ void pass_diag(amp_t (&x)[16], const cplx (&d)[4], const PassCtl &ct, Sel sel) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (pass_skips<CTL>(c, ct)) continue;
        pass_put<CTL>(x[c], cmul_diag(d[sel(c)], x[c]), ct);
    }
}

__device__ __forceinline__ cplx pass_pick(bool s, cplx one, cplx zero) {
    return cplx{s ? one.re : zero.re, s ? one.im : zero.im};
}

template <int CTL>
__device__ __forceinline__ void pass_gate16(amp_t (&x)[16], const PassGate &pg, uint32_t g0) {
    const double *__restrict__ m = pg.m;
    const PassCtl ct = {pg.rc, (g0 & pg.tc) == pg.tc};
#define QSV_PASS_D4(FORM, P0, P1) case (FORM) * 16 + (P0) * 4 + (P1): pass_dense<CTL, 4, (FORM) - PASS_D4, P0, P1>(x, m, ct); break;
#define QSV_PASS_D4_BOTH(FORM, LO, HI) QSV_PASS_D4(FORM, LO, HI) QSV_PASS_D4(FORM, HI, LO)
    switch (pg.form * 16 + pg.code) {     // wave-uniform (scalar loads)
        case PASS_D2 * 16 + 0: pass_dense<CTL, 2, 0, 0, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 1: pass_dense<CTL, 2, 0, 1, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 2: pass_dense<CTL, 2, 0, 2, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 3: pass_dense<CTL, 2, 0, 3, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 0: pass_dense<CTL, 2, 1, 0, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 1: pass_dense<CTL, 2, 1, 1, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 2: pass_dense<CTL, 2, 1, 2, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 3: pass_dense<CTL, 2, 1, 3, 0>(x, m, ct); break;
        QSV_PASS_D4_BOTH(PASS_D4, 0, 1) QSV_PASS_D4_BOTH(PASS_D4, 0, 2) QSV_PASS_D4_BOTH(PASS_D4, 0, 3)
        QSV_PASS_D4_BOTH(PASS_D4, 1, 2) QSV_PASS_D4_BOTH(PASS_D4, 1, 3) QSV_PASS_D4_BOTH(PASS_D4, 2, 3)
        QSV_PASS_D4_BOTH(PASS_D4X, 0, 1) QSV_PASS_D4_BOTH(PASS_D4X, 0, 2) QSV_PASS_D4_BOTH(PASS_D4X, 0, 3)
        QSV_PASS_D4_BOTH(PASS_D4X, 1, 2) QSV_PASS_D4_BOTH(PASS_D4X, 1, 3) QSV_PASS_D4_BOTH(PASS_D4X, 2, 3)
        // one low and one high target: the low one (kernel bit 0) has the smaller tile index, so the smaller register bit
        QSV_PASS_D4(PASS_D4HL, 0, 1) QSV_PASS_D4(PASS_D4HL, 0, 2) QSV_PASS_D4(PASS_D4HL, 0, 3)
        QSV_PASS_D4(PASS_D4HL, 1, 2) QSV_PASS_D4(PASS_D4HL, 1, 3) QSV_PASS_D4(PASS_D4HL, 2, 3)
        case PASS_PAIR * 16 + 0 * 4 + 1: pass_pair<CTL, 0, 1>(x, ct); break;
        case PASS_PAIR * 16 + 0 * 4 + 2: pass_pair<CTL, 0, 2>(x, ct); break;
        case PASS_PAIR * 16 + 0 * 4 + 3: pass_pair<CTL, 0, 3>(x, ct); break;
        case PASS_PAIR * 16 + 1 * 4 + 2: pass_pair<CTL, 1, 2>(x, ct); break;
        case PASS_PAIR * 16 + 1 * 4 + 3: pass_pair<CTL, 1, 3>(x, ct); break;
        case PASS_PAIR * 16 + 2 * 4 + 3: pass_pair<CTL, 2, 3>(x, ct); break;
        case PASS_DIAG_T * 16: {       // both selector bits are thread bits: one factor per thread
            const bool s0 = (g0 >> pg.tz0) & 1, s1 = (g0 >> pg.tz1) & 1;
            const cplx d[4] = {pass_pick(s0, pass_pick(s1, cplx{m[6], m[7]}, cplx{m[4], m[5]}),
                                         pass_pick(s1, cplx{m[2], m[3]}, cplx{m[0], m[1]})), {}, {}, {}};
            pass_diag<CTL>(x, d, ct, [](int) { return 0; });
            break;
        }
#define QSV_PASS_R1(P) case PASS_DIAG_R1 * 16 + (P): { \
            const cplx d[4] = {{m[0], m[1]}, {m[2], m[3]}, {}, {}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (c >> (P)) & 1; }); break; }
        QSV_PASS_R1(0) QSV_PASS_R1(1) QSV_PASS_R1(2) QSV_PASS_R1(3)
#define QSV_PASS_R2(P0, P1) case PASS_DIAG_R2 * 16 + (P0) * 4 + (P1): { \
            const cplx d[4] = {{m[0], m[1]}, {m[2], m[3]}, {m[4], m[5]}, {m[6], m[7]}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (((c >> (P0)) & 1) << 1) | ((c >> (P1)) & 1); }); break; }
        QSV_PASS_R2(0, 1) QSV_PASS_R2(0, 2) QSV_PASS_R2(0, 3) QSV_PASS_R2(1, 2) QSV_PASS_R2(1, 3) QSV_PASS_R2(2, 3)
#define QSV_PASS_M(P) case PASS_DIAG_M * 16 + (P): { \
            const bool s = (g0 >> pg.tz0) & 1; \
            const cplx d[4] = {pass_pick(s, cplx{m[2], m[3]}, cplx{m[0], m[1]}), pass_pick(s, cplx{m[6], m[7]}, cplx{m[4], m[5]}), {}, {}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (c >> (P)) & 1; }); break; }
        QSV_PASS_M(0) QSV_PASS_M(1) QSV_PASS_M(2) QSV_PASS_M(3)
        default: break;       // qsvk_pass builds no other record
    }
#undef QSV_PASS_D4
#undef QSV_PASS_D4_BOTH
#undef QSV_PASS_R1
#undef QSV_PASS_R2
#undef QSV_PASS_M
}

__device__ __forceinline__ void pass_gate16(amp_t (&x)[16], const PassGate &pg, uint32_t g0) {
    switch (pg.ctl) {                     // wave-uniform
        case PASS_CTL_NONE: pass_gate16<PASS_CTL_NONE>(x, pg, g0); break;
        case PASS_CTL_REG: pass_gate16<PASS_CTL_REG>(x, pg, g0); break;
        default: pass_gate16<PASS_CTL_THREAD>(x, pg, g0); break;
    }
}

// omask[]: the gates' omask fields packed, padded with zeros to a multiple of 8 entries (read eight at a time).
template <bool NT>
__global__ __launch_bounds__(PASS_THREADS) void k_pass_tile(amp_t *__restrict__ a, const PassArgs pa,
                                                            const PassGate *__restrict__ gates, int n_gates,
                                                            const PassGroup *__restrict__ groups, int n_groups,
                                                            const uint64_t *__restrict__ omask) {
    __shared__ amp_t tile[PASS_TILE];      // [row][64 lanes]: LDS index = tile index (bits 0..5 lane, 6..11 row)
    const BigArgs &g = pa.g;
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RPW = PASS_ROWS_PER_WAVE;
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    uint64_t base = g.w0 + tile_id;        // deposit() with the trip count known: pos[] arrives in wide loads
#pragma unroll
    for (int j = 0; j < qsv_plan::TILE_BITS; ++j) base = insert_zero(base, static_cast<int>(g.pos[j]));
    base |= g.or_mask;
    // this wave's rows are q RPW + i: the wave's own offset, plus those of the bits of i when a row is addressed (they are
    // not kept in scalar registers from the load to the store: sixteen 64-bit offsets would be a third of them)
    static_assert(RPW == 16 && PASS_ROWS == 64, "four row bits from i, two from the wave number");
    uint64_t row0 = base + (static_cast<uint64_t>(q & 1) << g.pos[10]) + (static_cast<uint64_t>(q >> 1) << g.pos[11]);
    auto row = [&](int i) {
        uint64_t r = row0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((i >> j) & 1) r += 1ull << g.pos[6 + j];
        return r;
    };
    auto request_tile = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll
        for (int i = 0; i < RPW; ++i)
            __builtin_amdgcn_global_load_lds(a + row(i) + lane, tile + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    };
    // With a gate that acts on every tile in the pass, the tile is requested before the gates' outside controls are
    // looked at, and that look happens under the loads.
    if (pa.every_tile) request_tile();
    uint64_t active = 0;                   // wave-uniform: bit i = gate i acts on this tile
    for (int i0 = 0; i0 < n_gates; i0 += 8) {
        uint64_t om[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) om[j] = omask[i0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) active |= static_cast<uint64_t>((base & om[j]) == om[j]) << (i0 + j);
    }
    active &= ~0ull >> (64 - n_gates);     // the padding reads as gates without outside controls
    if (!pa.every_tile) {
        if (!active) return;
        request_tile();
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < n_groups; ++p) {
        const PassGroup &gr = groups[p];
        if (!(active & gr.gates)) continue;     // no gate of the group acts on this tile: no LDS trip
        const int q0 = gr.q[0], q1 = gr.q[1], q2 = gr.q[2], q3 = gr.q[3];
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
        for (int i = gr.first; i < gr.first + gr.count; ++i)
            if ((active >> i) & 1) pass_gate16(x, gates[i], g0);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)] = x[c];
        __syncthreads();
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // Without this the compiler keeps the sixteen row offsets of the load alive for the store: 32 SGPRs across the gate
    // loop, beside the 64 of a 4 x 4 matrix -- the build that did so spilled SGPRs into v_writelane / v_readlane in the
    // 2-qubit bodies (sgpr_spill_count 21 in the kernel's metadata; 0 with it).  row0 comes out as it went in.
    asm volatile("" : "+s"(row0));
#endif
#pragma unroll
    for (int i = 0; i < RPW; ++i) st<NT>(a + row(i) + lane, tile[(q * RPW + i) * 64 + lane]);
}

bool qsvk_op_exact(const QsvOp &op) {
    if (op.kind == QSV_OP_PAIR) return true;
    auto unit = [](double re, double im) { return im == 0.0 && (re == 1.0 || re == -1.0); };
    if (op.kind == QSV_OP_PHASE) return unit(op.m[0], op.m[1]);
    if (op.kind == QSV_OP_DIAG) {
        for (int i = 0; i < (1 << op.k); ++i)
            if (!unit(op.m[2 * i], op.m[2 * i + 1])) return false;
        return true;
    }
    // dense: one +-1 per row and per column, zeros elsewhere (every output is one input, negated or not)
    const int D = 1 << op.k;
    int per_col[4] = {0, 0, 0, 0};
    for (int r = 0; r < D; ++r) {
        int nz = 0;
        for (int c = 0; c < D; ++c) {
            const double re = op.m[2 * (r * D + c)], im = op.m[2 * (r * D + c) + 1];
            if (re == 0.0 && im == 0.0) continue;
            if (!unit(re, im)) return false;
            ++nz;
            ++per_col[c];
        }
        if (nz != 1) return false;
    }
    for (int c = 0; c < D; ++c)
        if (per_col[c] != 1) return false;
    return true;
}

int qsvk_run_op(qsv_state *st, const QsvOp &op) {
    switch (op.kind) {
        case QSV_OP_DENSE: return qsvk_dense(st, op.k, op.bits, op.nctrl, op.cbits, op.m);
        case QSV_OP_PAIR: return qsvk_pair_exchange(st, op.bits[0], op.bits[1]);
        case QSV_OP_DIAG: return qsvk_diag(st, op.k, op.bits, op.nctrl, op.cbits, op.m);
        case QSV_OP_PHASE: return qsvk_phase(st, op.nctrl, op.cbits, op.m[0], op.m[1]);
        default: return qsv_fail(QSV_EINVAL, "internal: unknown queued gate kind");
    }
}

// One k_pass_tile launch for `count` queued gates (in application order) on the tiles spanned by bits 0..5 and tile_high.
int qsvk_pass(qsv_state *st, const QsvOp *const *ops, int count, uint64_t tile_high) {
    const uint64_t low = (1ull << QSV_LANE_BITS) - 1;
    if (count < 1 || count > qsv_plan::MAX_PASS_GATES || st->n < qsv_plan::TILE_BITS || (tile_high & low) ||
        __builtin_popcountll(tile_high) != qsv_plan::HIGH_BITS || (tile_high >> st->n))
        return qsv_fail(QSV_EINVAL, "internal: malformed gate pass");
    const PassRecords pr = pass_records(ops, count, tile_high, st->amps);
    if (pr.status == PassRecords::TARGET_OUTSIDE_TILE) return qsv_fail(QSV_EINVAL, "internal: gate target outside its pass's tile");
    if (pr.status == PassRecords::TARGET_OUTSIDE_GROUP) return qsv_fail(QSV_EINVAL, "internal: gate target outside its group's register bits");
    // staged: the records, then the groups with the packed omasks behind them (padded to the eight the kernel reads at a time)
    const size_t grp_bytes = sizeof(PassGroup) * pr.grp.size(), omask_count = (pr.omask.size() + 7) / 8 * 8;
    std::vector<char> tail(grp_bytes + sizeof(uint64_t) * omask_count, 0);
    std::memcpy(tail.data(), pr.grp.data(), grp_bytes);
    std::memcpy(tail.data() + grp_bytes, pr.omask.data(), sizeof(uint64_t) * pr.omask.size());
    StageRef staged;
    int rc = qsvk_stage(st, pr.rec.data(), sizeof(PassGate) * pr.rec.size(), tail.data(), tail.size(), &staged);
    if (rc) return rc;
    const PassGate *dev_g = reinterpret_cast<const PassGate *>(staged.dev);
    const PassGroup *dev_p = reinterpret_cast<const PassGroup *>(staged.dev + qsv_pad16(sizeof(PassGate) * pr.rec.size()));
    const uint64_t *dev_o = reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(dev_p) + grp_bytes);
    const int n_groups = static_cast<int>(pr.grp.size());
    const std::vector<int> tile_bits(pr.tile_bits, pr.tile_bits + qsv_plan::TILE_BITS);
    PassArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.g = with_enumeration<BigArgs>(enumeration(st->amps >> qsv_plan::TILE_BITS, tile_bits));   // tiles: the index with every tile bit taken out
    pa.g.regions = regions_or(st, 8);
    pa.every_tile = pr.every_tile ? 1u : 0u;
    const bool nt = st->nontemporal != 0;
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_pass_tile<%s>", nt ? "true" : "false");
    rc = launch_ranges(pa.g, DISPATCH_TILES, [&](uint64_t tiles) {
        const dim3 gd(static_cast<unsigned>(tiles)), bd(PASS_THREADS);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_pass_tile<NT.value>, gd, bd, 0, st->stream, st->data, pa, dev_g, count, dev_p, n_groups, dev_o); });
    });
    return rc ? rc : qsvk_stage_done(st, staged);
}

// k = 5 (complex matrices) and k = 6 on the matrix cores (k_dense_mfma).  bits[j] = bit position of matrix leg j (leg 0
// most significant).
static int launch_dense_mfma(qsv_state *st, int k, const int *bits, const double *m_user, const FormChoice &f) {
    const int D = 1 << k;
    // A wave's 16 lanes li are the 16 lowest free index values and its 4 lanes lk the two lowest target bits, so a
    // wave-instruction covers whole 128-byte lines wherever the targets sit, unless bits 0, 1 AND 2 are all targets
    // (then it covers half lines, and the other half follows in the next instruction of the same wave): 2.9-3.1 ms at
    // every placement.  (Round 2 first moved low targets away with a qubit permutation before and after: 6.2 ms.)
    std::vector<int> sorted(bits, bits + k);
    std::sort(sorted.begin(), sorted.end());
    // register / matrix index c: bit i <-> sorted[i]
    const std::vector<uint64_t> off = offsets(sorted);
    const std::vector<double> m = matrix(f.realm ? MAT_COLUMNS_REAL : MAT_COLUMNS, D, m_user, user_index(k, bits, sorted.data()).data());
    StageRef staged;
    int rc = qsvk_stage(st, m.data(), sizeof(double) * m.size(), off.data(), sizeof(uint64_t) * D, &staged);
    if (rc) return rc;
    const double *dev_m = reinterpret_cast<const double *>(staged.dev);
    const uint64_t *dev_off = reinterpret_cast<const uint64_t *>(staged.dev + qsv_pad16(sizeof(double) * m.size()));
    const Mfma6Args g = with_enumeration<Mfma6Args>(enumeration(st->amps >> k, sorted));
    const bool nt = st->nontemporal != 0;
    const size_t lds = sizeof(double) * m.size() + sizeof(uint64_t) * D;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, st->device);  // 256 if the query fails
    const uint64_t wave_tiles = g.W / 16;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((wave_tiles + 3) / 4, ((k == 6 && !f.realm) ? 2ull : 3ull) * cus));
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_dense_mfma<%d, %s, %s%s>", k, nt ? "true" : "false",
             f.realm ? "true" : "false", f.m3 ? ", true" : "");
    auto launch = [&](auto kernel) -> int {
        QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(QSV_BLOCK), lds, st->stream, st->data, g, dev_m, dev_off);
        return check_launch();
    };
    rc = with_int<5, 6>(k, [&](auto K) { return with_bool(f.realm, [&](auto REAL) { return with_bool(nt, [&](auto NT) {
        if constexpr (!REAL.value) {
            if (f.m3) return launch(k_dense_mfma<K.value, NT.value, false, true>);
        }
        return launch(k_dense_mfma<K.value, NT.value, REAL.value>);
    }); }); });
    return rc ? rc : qsvk_stage_done(st, staged);
}

int qsvk_generic(qsv_state *st, int k, const int *bits, const double *m_user) {
    if (k < 1 || k > QSV_MAX_K) return qsv_fail(QSV_EINVAL, "generic gate: k must be in 1..6");
    const FormChoice f = choose_form(st->n, st->amps, k, bits, is_real(1 << k, m_user),
                                     FormOptions{st->kq_variant, st->complex_product, mtile_default()});
    if (f.form == FORM_MFMA) return launch_dense_mfma(st, k, bits, m_user, f);
    if (f.form != FORM_GATHER) return launch_dense_big(st, k, bits, m_user, f);
    const size_t bytes = sizeof(double) * 2ull << (2 * k);
    StageRef staged;
    int rc = qsvk_stage(st, m_user, bytes, nullptr, 0, &staged);
    if (rc) return rc;
    const double *dev_m = reinterpret_cast<const double *>(staged.dev);
    GenericArgs g;
    std::memset(&g, 0, sizeof(g));
    g.K = k;
    g.W = st->amps >> k;
    std::vector<int> sorted(bits, bits + k);
    std::sort(sorted.begin(), sorted.end());
    for (int j = 0; j < k; ++j) {
        g.sorted_pos[j] = static_cast<uint8_t>(sorted[j]);
        g.leg_pos[j] = static_cast<uint8_t>(bits[j]);
    }
    const int grid = grid_for(g.W, QSV_BLOCK, 4096);
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_generic<%d>", k);
    switch (k) {
        case 1: hipLaunchKernelGGL((k_generic<1>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
        case 2: hipLaunchKernelGGL((k_generic<2>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
        case 3: hipLaunchKernelGGL((k_generic<3>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
        case 4: hipLaunchKernelGGL((k_generic<4>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
        case 5: hipLaunchKernelGGL((k_generic<5>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
        default: hipLaunchKernelGGL((k_generic<6>), dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); break;
    }
    rc = check_launch();
    if (rc) return rc;
    return qsvk_stage_done(st, staged);
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

int qsvk_copy(amp_t *dst, const amp_t *src, uint64_t amps, hipStream_t stream) {
    static const int mode = [] { const char *e = getenv("QSV_COPY_MODE"); return e ? atoi(e) : 1; }();
    static const int regions = [] { const char *e = getenv("QSV_COPY_REGIONS"); return e ? atoi(e) : 0; }();
    const uint64_t per_block = mode == 0 ? QSV_BLOCK * COPY_ITEMS : QSV_BLOCK;
    const uint64_t bulk = amps / per_block * per_block;
    for (uint64_t done = 0; done < bulk;) {   // an AQL dispatch counts work-items in 32 bits
        const uint64_t blocks = std::min<uint64_t>((bulk - done) / per_block, 1ull << 23);
        const dim3 gd(static_cast<unsigned>(blocks)), bd(QSV_BLOCK);
        if (mode == 0) hipLaunchKernelGGL(k_copy<0>, gd, bd, 0, stream, dst + done, src + done, regions);
        else if (mode == 1) hipLaunchKernelGGL(k_copy<1>, gd, bd, 0, stream, dst + done, src + done, regions);
        else hipLaunchKernelGGL(k_copy<2>, gd, bd, 0, stream, dst + done, src + done, regions);
        done += blocks * per_block;
    }
    if (bulk < amps) {
        hipError_t e = hipMemcpyAsync(dst + bulk, src + bulk, sizeof(amp_t) * (amps - bulk), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return qsv_fail(QSV_EHIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    }
    return check_launch();
}

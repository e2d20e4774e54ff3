// Dense k-qubit gates, k = 3..6 (and k_generic, the gather form every k falls back to on tiny registers): the forms
// qsv_layout::choose_form picks among -- register-blocked with wave shuffles (k_dense_big), line-granular through LDS rows
// (k_dense_lds), workgroup tile (k_dense_tile), tile-fed matrix cores (k_dense_mtile5), matrix cores (k_dense_mfma) -- and
// qsvk_generic, which launches them.  How the gates touch memory is described at the head of qsv_gate12.hip.

#include "qsv_internal.h"
#include "qsv_device.h"
#include "qsv_layout.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace qsv_layout;   // the argument and record types of the kernels, and the host-side tables the launchers fill them from

namespace {

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

}  // namespace

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
    with_int<1, 6>(k, [&](auto K) { hipLaunchKernelGGL(k_generic<K.value>, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, g, dev_m); });
    rc = check_launch();
    if (rc) return rc;
    return qsvk_stage_done(st, staged);
}

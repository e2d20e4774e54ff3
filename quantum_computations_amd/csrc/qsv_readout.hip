// Read-out and reshaping kernels of the qubit register (gfx950, wave64): measurement, collapse, insertion, permutation,
// reductions, reduced density matrices, sampling and fills, with their launchers.  The host-side index arithmetic of the
// launchers lives in qsv_readout_layout.h.

#include "qsv_device.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace qsv_readout_layout;   // the argument types of the kernels, and the host-side tables the launchers fill them from

namespace {

// ----------------------------------------------------------------------------------------------------
// Reductions, measurement, insertion, permutation, fills.
// ----------------------------------------------------------------------------------------------------
// partials[2*block + s] = sum over this block's pairs of |eig_s[0] a0 + eig_s[1] a1|^2
__global__ __launch_bounds__(QSV_BLOCK) void k_measure_probs(const amp_t *__restrict__ a, uint64_t pairs, int bit,
                                                            cplx e00, cplx e01, cplx e10, cplx e11,
                                                            double *__restrict__ partials) {
    double p0 = 0.0, p1 = 0.0;
    const uint64_t s = 1ull << bit;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; w < pairs;
         w += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t i0 = insert_zero(w, bit);
        const amp_t a0 = a[i0], a1 = a[i0 + s];
        const amp_t r0 = cfma(e01, a1, cmul(e00, a0));
        const amp_t r1 = cfma(e11, a1, cmul(e10, a0));
        p0 += r0.x * r0.x + r0.y * r0.y;
        p1 += r1.x * r1.x + r1.y * r1.y;
    }
    block_sum2(p0, p1);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = p0;
        partials[2 * blockIdx.x + 1] = p1;
    }
}

// out[w] = scale * (e0 a[i0] + e1 a[i1]): the (n-1)-qubit post-measurement ket.
__global__ __launch_bounds__(QSV_BLOCK) void k_collapse(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                       uint64_t pairs, int bit, cplx e0, cplx e1, double scale) {
    const uint64_t s = 1ull << bit;
    for (uint64_t w = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; w < pairs;
         w += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t i0 = insert_zero(w, bit);
        amp_t r = cfma(e1, a[i0 + s], cmul(e0, a[i0]));
        r.x *= scale;
        r.y *= scale;
        out[w] = r;
    }
}

// out[j] = amp[bit(j)] * a[j with the bit removed]: kron(state, new) + move (gates.py:149-152).
__global__ __launch_bounds__(QSV_BLOCK) void k_insert(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                     uint64_t out_amps, int bit, cplx c0, cplx c1) {
    for (uint64_t j = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; j < out_amps;
         j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t low = j & ((1ull << bit) - 1ull);
        const uint64_t src = ((j >> (bit + 1)) << bit) | low;
        out[j] = cmul(((j >> bit) & 1ull) ? c1 : c0, a[src]);
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_permute(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                      uint64_t amps, const PermArgs g) {
    for (uint64_t j = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; j < amps;
         j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        uint64_t src = 0;
        for (int b = 0; b < g.n; ++b) src |= ((j >> b) & 1ull) << g.src_bit[b];
        out[j] = a[src];
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_norm2(const amp_t *__restrict__ a, uint64_t amps,
                                                    double *__restrict__ partials) {
    double s = 0.0, unused = 0.0;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const amp_t v = a[i];
        s += v.x * v.x + v.y * v.y;
    }
    block_sum2(s, unused);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = s;
        partials[2 * blockIdx.x + 1] = 0.0;
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_inner(const amp_t *__restrict__ a, const amp_t *__restrict__ b,
                                                    uint64_t amps, double *__restrict__ partials) {
    double re = 0.0, im = 0.0;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const amp_t x = a[i], y = b[i];
        re += x.x * y.x + x.y * y.y;  // conj(x) * y
        im += x.x * y.y - x.y * y.x;
    }
    block_sum2(re, im);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = re;
        partials[2 * blockIdx.x + 1] = im;
    }
}

// Sampling, pass 1: chunk_sums[c] = sum of |amp|^2 over chunk c (SAMPLE_CHUNK consecutive amplitudes per workgroup).
constexpr int SAMPLE_CHUNK = 4096;

// |amp|^2 as BOTH passes form it: written with fma so that no pass is left to the compiler's contraction (pass 1 adds the
// weight to a sum in the same statement, pass 2 stores it first) -- a weight is the same double wherever it is formed.
__device__ __forceinline__ double sample_weight(amp_t v) { return fma(v.x, v.x, v.y * v.y); }

__global__ __launch_bounds__(QSV_BLOCK) void k_chunk_sums(const amp_t *__restrict__ a, uint64_t amps,
                                                         double *__restrict__ chunk_sums) {
    const uint64_t chunks = (amps + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        double s = 0.0, unused = 0.0;
        // thread t owns SAMPLE_CHUNK / QSV_BLOCK consecutive amplitudes: the same split pass 2 walks
        constexpr int PER = SAMPLE_CHUNK / QSV_BLOCK;
        const uint64_t first = c * SAMPLE_CHUNK + static_cast<uint64_t>(threadIdx.x) * PER;
        for (int k = 0; k < PER; ++k)
            if (first + k < amps) s += sample_weight(a[first + k]);
        __syncthreads();  // block_sum2 reuses its shared scratch across iterations
        block_sum2(s, unused);
        if (threadIdx.x == 0) chunk_sums[c] = s;
    }
}

// Sampling, pass 2: one workgroup per shot walks its chunk and returns the first index whose running sum of |amp|^2
// exceeds `residual`; where rounding leaves no such index -- this walk and pass 1 add the same weights in different
// orders -- the last one of positive weight, never an amplitude of weight zero.  sample_walk of qsv_readout_layout.h is
// this rule on the host, step for step.
__global__ __launch_bounds__(QSV_BLOCK) void k_sample_in_chunk(const amp_t *__restrict__ a, uint64_t amps,
                                                              const uint64_t *__restrict__ chunk_of_shot,
                                                              const double *__restrict__ residual_of_shot,
                                                              uint64_t *__restrict__ out) {
    __shared__ double part[QSV_BLOCK];
    __shared__ double before;      // the running sum in front of the owner thread
    __shared__ int owner_thread;   // the thread that holds the answer
    __shared__ int crossed;        // the thread sums crossed the residual (else: the last thread of positive sum)
    constexpr int PER = SAMPLE_CHUNK / QSV_BLOCK;
    const uint64_t c = chunk_of_shot[blockIdx.x];
    const double residual = residual_of_shot[blockIdx.x];
    const uint64_t first = c * SAMPLE_CHUNK + static_cast<uint64_t>(threadIdx.x) * PER;
    double mine[PER];
    double s = 0.0;
    for (int k = 0; k < PER; ++k) {
        const double p = first + k < amps ? sample_weight(a[first + k]) : 0.0;
        mine[k] = p;
        s += p;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        int owner = -1, last = -1;
        for (int t = 0; t < QSV_BLOCK; ++t) {
            const double sum = part[t];
            if (sum > 0.0) last = t;
            if (run + sum > residual) {
                owner = t;
                break;
            }
            run += sum;
        }
        before = run;
        crossed = owner >= 0;
        owner_thread = owner >= 0 ? owner : (last < 0 ? 0 : last);
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) == owner_thread) {
        double run = before;
        int slot = -1, last = -1;
        for (int k = 0; k < PER; ++k) {
            if (mine[k] > 0.0) last = k;
            if (crossed && run + mine[k] > residual) {
                slot = k;
                break;
            }
            run += mine[k];
        }
        if (slot < 0) slot = last < 0 ? 0 : last;
        uint64_t idx = first + slot;
        if (idx >= amps) idx = amps - 1;   // a chunk of zero weight only: sample_chunks never picks one
        out[blockIdx.x] = idx;
    }
}

__global__ void k_gather_prob(const amp_t *__restrict__ a, const uint64_t *__restrict__ idx, int count,
                              double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const amp_t v = a[idx[i]];
        out[i] = v.x * v.x + v.y * v.y;
    }
}

__global__ __launch_bounds__(QSV_BLOCK) void k_scale(amp_t *__restrict__ a, uint64_t amps, cplx c) {
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        a[i] = cmul(c, a[i]);
}

__global__ __launch_bounds__(QSV_BLOCK) void k_zero(amp_t *__restrict__ a, uint64_t amps, uint64_t one_at) {
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        a[i] = amp_t{i == one_at ? 1.0 : 0.0, 0.0};
}

// splitmix64: counter-based, so a sharded register can be filled shard by shard from global indices.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(QSV_BLOCK) void k_fill_random(amp_t *__restrict__ a, uint64_t amps, uint64_t seed,
                                                          uint64_t index_offset, double *__restrict__ partials) {
    double s = 0.0, unused = 0.0;
    const uint64_t key = splitmix64(seed);
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < amps;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t g = i + index_offset;
        const uint64_t r1 = splitmix64(key ^ (2 * g)), r2 = splitmix64(key ^ (2 * g + 1));
        const double u1 = (static_cast<double>(r1 >> 11) + 0.5) * 0x1.0p-53;  // (0, 1)
        const double u2 = (static_cast<double>(r2 >> 11) + 0.5) * 0x1.0p-53;
        const double rad = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincos(6.283185307179586476925286766559 * u2, &sn, &cs);
        const amp_t v = {rad * cs, rad * sn};
        a[i] = v;
        s += v.x * v.x + v.y * v.y;
    }
    block_sum2(s, unused);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = s;
        partials[2 * blockIdx.x + 1] = 0.0;
    }
}


// ----------------------------------------------------------------------------------------------------
// Streaming forms of the read-out / reshaping kernels (registers of at least 2^14 amplitudes; the plain grid-stride
// forms above stay for smaller ones).  Common shape: one work item = 64 consecutive amplitudes per wave-instruction,
// ITEMS independent items per thread in flight, nontemporal accesses (every amplitude is touched once), and a target
// bit below 6 is resolved inside the wave -- the partner amplitude comes from __shfl_xor, compaction / expansion by
// one qubit is a lane gather -- so that every global access is a whole 1 KiB segment whatever the bit.
// ----------------------------------------------------------------------------------------------------
constexpr int RO_ITEMS = 4;          // the reductions (k_measure_probs_s): four items per thread and trip

// partials[2*block + s] = sum over this block's pairs of |eig_s[0] a0 + eig_s[1] a1|^2   (M.apply, gates.py:173-183)
template <bool LOW>
__global__ __launch_bounds__(QSV_BLOCK) void k_measure_probs_s(const amp_t *__restrict__ a, uint64_t amps, int bit,
                                                               cplx e00, cplx e01, cplx e10, cplx e11,
                                                               double *__restrict__ partials) {
    double p0 = 0.0, p1 = 0.0;
    const uint64_t s = 1ull << bit;
    if constexpr (LOW) {
        // natural order: a lane whose bit is 0 holds a0 and fetches a1 from its partner (and accumulates outcome 0),
        // a lane whose bit is 1 holds a1, fetches a0 and accumulates outcome 1: no lane idles, no amplitude is read twice
        const bool up = (threadIdx.x >> bit) & 1;
        const cplx mine = up ? e11 : e00, theirs = up ? e10 : e01;
        double acc = 0.0;
        const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK * RO_ITEMS;
        for (uint64_t i0 = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) * RO_ITEMS + threadIdx.x; i0 < amps; i0 += stride) {
            amp_t v[RO_ITEMS];
#pragma unroll
            for (int u = 0; u < RO_ITEMS; ++u) v[u] = __builtin_nontemporal_load(a + i0 + u * QSV_BLOCK);
#pragma unroll
            for (int u = 0; u < RO_ITEMS; ++u) {
                const amp_t r = cfma(theirs, shfl_xor_amp(v[u], 1 << bit), cmul(mine, v[u]));
                acc += r.x * r.x + r.y * r.y;
            }
        }
        p0 = up ? 0.0 : acc;
        p1 = up ? acc : 0.0;
    } else {
        const uint64_t pairs = amps >> 1;
        const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK * RO_ITEMS;
        for (uint64_t w0 = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) * RO_ITEMS + threadIdx.x; w0 < pairs; w0 += stride) {
            amp_t lo[RO_ITEMS], hi[RO_ITEMS];
#pragma unroll
            for (int u = 0; u < RO_ITEMS; ++u) {
                const uint64_t i = insert_zero(w0 + u * QSV_BLOCK, bit);
                lo[u] = __builtin_nontemporal_load(a + i);
                hi[u] = __builtin_nontemporal_load(a + i + s);
            }
#pragma unroll
            for (int u = 0; u < RO_ITEMS; ++u) {
                const amp_t r0 = cfma(e01, hi[u], cmul(e00, lo[u]));
                const amp_t r1 = cfma(e11, hi[u], cmul(e10, lo[u]));
                p0 += r0.x * r0.x + r0.y * r0.y;
                p1 += r1.x * r1.x + r1.y * r1.y;
            }
        }
    }
    block_sum2(p0, p1);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = p0;
        partials[2 * blockIdx.x + 1] = p1;
    }
}

// out[w] = scale * (e0 a[i0] + e1 a[i0 + s]), i0 = w with a zero inserted at `bit`.
template <bool LOW, int ITEMS>
__global__ __launch_bounds__(QSV_BLOCK) void k_collapse_s(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                          uint64_t pairs, int bit, cplx e0, cplx e1, double scale) {
    const cplx f0 = {e0.re * scale, e0.im * scale}, f1 = {e1.re * scale, e1.im * scale};
    const uint64_t w0 = (blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + (threadIdx.x & ~63u)) * ITEMS + (threadIdx.x & 63);
    if constexpr (LOW) {
        // a wave turns 2 * ITEMS rows of 64 amplitudes into ITEMS rows of 64 results: the pair sum lands in the
        // lanes whose bit is 0, and output lane l gathers it from lane insert_zero(l & 31, bit) of row l >> 5
        const int lane = threadIdx.x & 63;
        const int src = static_cast<int>(insert_zero(static_cast<uint64_t>(lane & 31), bit));
        amp_t v[2 * ITEMS];
#pragma unroll
        for (int u = 0; u < 2 * ITEMS; ++u) v[u] = __builtin_nontemporal_load(a + 2 * (w0 - lane) + u * 64 + lane);
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            const amp_t ra = cfma(f1, shfl_xor_amp(v[2 * u], 1 << bit), cmul(f0, v[2 * u]));
            const amp_t rb = cfma(f1, shfl_xor_amp(v[2 * u + 1], 1 << bit), cmul(f0, v[2 * u + 1]));
            const amp_t ga = shfl_amp(ra, src), gb = shfl_amp(rb, src);
            __builtin_nontemporal_store(lane < 32 ? ga : gb, out + w0 + u * 64);
        }
    } else {
        const uint64_t s = 1ull << bit;
        amp_t lo[ITEMS], hi[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            const uint64_t i = insert_zero(w0 + u * 64, bit);
            lo[u] = __builtin_nontemporal_load(a + i);
            hi[u] = __builtin_nontemporal_load(a + i + s);
        }
#pragma unroll
        for (int u = 0; u < ITEMS; ++u)
            __builtin_nontemporal_store(cfma(f1, hi[u], cmul(f0, lo[u])), out + w0 + u * 64);
    }
}

// out[j] = amp[bit(j)] * a[j with the bit removed]
template <bool LOW, int ITEMS>
__global__ __launch_bounds__(QSV_BLOCK) void k_insert_s(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                        uint64_t in_amps, int bit, cplx c0, cplx c1) {
    const uint64_t w0 = (blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + (threadIdx.x & ~63u)) * ITEMS + (threadIdx.x & 63);
    amp_t v[ITEMS];
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) v[u] = __builtin_nontemporal_load(a + w0 + u * 64);
    if constexpr (LOW) {
        // a row of 64 inputs becomes two rows of 64 outputs: output lane l of row h reads input lane 32 h + (l without
        // its `bit`) and takes the factor of its own bit
        const int lane = threadIdx.x & 63;
        const int from = static_cast<int>(((static_cast<uint32_t>(lane) >> (bit + 1)) << bit) | (lane & ((1 << bit) - 1)));
        const cplx c = ((lane >> bit) & 1) ? c1 : c0;
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            const uint64_t o = 2 * (w0 - lane + u * 64) + lane;
            __builtin_nontemporal_store(cmul(c, shfl_amp(v[u], from)), out + o);
            __builtin_nontemporal_store(cmul(c, shfl_amp(v[u], 32 + from)), out + o + 64);
        }
    } else {
        const uint64_t s = 1ull << bit;
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            const uint64_t o = insert_zero(w0 + u * 64, bit);
            __builtin_nontemporal_store(cmul(c0, v[u]), out + o);
            __builtin_nontemporal_store(cmul(c1, v[u]), out + o + s);
        }
    }
}

// Qubit permutation: out[j] = a[p(j)], p moves index bits.  A wave owns a tile of 64 amplitudes that is 8 whole
// 128-byte lines on BOTH sides: the tile's six index bits are the destination bits 0..2 (inside a line), the destination
// bits fed by source bits 0..2, and filler bits.  Stores are consecutive within each line; loads hit 8 whole source lines
// in some lane order -- no LDS and no shuffle, the coalescer sees complete lines either way.  The tile's base addresses
// are wave-uniform: the destination base is the tile number with zeros inserted at the tile's bit positions, the source
// base is that number pushed through the bit permutation one byte at a time (256-entry tables, scalar loads).
template <int ITEMS>
__global__ __launch_bounds__(QSV_BLOCK) void k_permute_s(const amp_t *__restrict__ a, amp_t *__restrict__ out,
                                                         const PermTileArgs g,
                                                         const uint64_t *__restrict__ lut /*[bytes][256]*/) {
    const int lane = threadIdx.x & 63;
    uint64_t dst_lane = 0, src_lane = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t b = (lane >> k) & 1;
        dst_lane |= b << g.tile_dst[k];
        src_lane |= b << g.tile_src[k];
    }
    // wave-uniform on purpose (readfirstlane): the per-tile address arithmetic below then runs on the scalar unit
    const uint64_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (QSV_BLOCK / 64) + (threadIdx.x >> 6));
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (QSV_BLOCK / 64);
    for (uint64_t t0 = wave * ITEMS; t0 < g.tiles; t0 += waves * ITEMS) {
        amp_t v[ITEMS];
        uint64_t dst[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            uint64_t d = t0 + u;
#pragma unroll
            for (int k = 0; k < 6; ++k) d = insert_zero(d, g.tile_dst[k]);
            uint64_t sidx = 0;
            for (int b = 0; b < g.bytes; ++b) sidx |= lut[b * 256 + ((d >> (8 * b)) & 255)];
            dst[u] = d | dst_lane;
            v[u] = amp_t{0.0, 0.0};
            if (t0 + u < g.tiles) v[u] = __builtin_nontemporal_load(a + (sidx | src_lane));
        }
#pragma unroll
        for (int u = 0; u < ITEMS; ++u)
            if (t0 + u < g.tiles) __builtin_nontemporal_store(v[u], out + dst[u]);
    }
}

// ----------------------------------------------------------------------------------------------------
// Reduced density matrix of k <= 6 kept qubits in ONE read pass:  rho[i][j] = sum_g psi[i, g] conj(psi[j, g]),
// g running over the 2^(n-k) settings of the other qubits.  That is X X^H for the (2^k x 2^(n-k)) matrix X -- a rank
// update with a tiny result -- and runs on the f64 matrix cores: a lane (i = lane & 15, kk = lane >> 4) loads ONE
// amplitude, row i of group 4 q + kk, and the same register pair serves as A[i][kk] and as B[kk][j] of
// v_mfma_f64_16x16x4_f64 (re = xr xr^T + xi xi^T, im = xi xr^T - xr xi^T).  T = 1, 2, 4 row tiles of 16 cover
// 2^k <= 16, 32, 64; only the upper triangle of tiles is accumulated (rho is Hermitian).  The sum is deterministic:
// waves add into their workgroup's LDS tile one after the other, workgroups write partials, a second launch adds
// the partials in index order.
// ----------------------------------------------------------------------------------------------------
// RDM_U quads of groups are loaded before the first MFMA of an iteration (a wave with a single 16-byte load in flight
// spends its life waiting for HBM: 0.25-1.3 TB/s in the first version of this kernel).  When 2^k < 16 the sixteen rows
// of the tile are shared by S = 16 / 2^k groups (row i = r + 2^k s): every lane still loads a different amplitude, the
// tile then holds S x S blocks of which only the S diagonal ones (same group on both sides) mean anything; the host adds
// those up.  (RDM_LOADS, which the launch plan needs too, is qsv_readout_layout.h's.)
template <int T>
__global__ __launch_bounds__(QSV_BLOCK) void k_rdm(const amp_t *__restrict__ a, const RdmArgs g,
                                                   const uint64_t *__restrict__ hoff,  // [16 T] row offsets
                                                   double *__restrict__ partials) {    // [grid][P][2][256]
    constexpr int P = T * (T + 1) / 2;
    constexpr int RDM_U = RDM_LOADS / T;
    __shared__ double red[P * 2 * 256];
    const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    const int S = T == 1 ? 16 / g.D : 1;                 // groups sharing the 16 rows of a tile (D = 1 never occurs)
    const uint64_t sub = T == 1 ? static_cast<uint64_t>(i / g.D) : 0;
    uint64_t row_off[T];
#pragma unroll
    for (int t = 0; t < T; ++t) row_off[t] = hoff[T == 1 ? i % g.D : 16 * t + i];
    // C independent accumulator sets: consecutive MFMAs never wait for one another's result (with one set per tile
    // pair the two updates of `re` and of `im` in a step are back-to-back dependent issues of a 64-cycle instruction)
    constexpr int C = RDM_U >= 2 ? 2 : 1;
    f64x4 re[C][P], im[C][P];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) re[c][p] = im[c][p] = f64x4{0.0, 0.0, 0.0, 0.0};
    // a step = 4 S groups = one MFMA k-slice per tile pair.  The host sizes the grid so that waves * RDM_U divides the
    // step count: every load below is unconditional.
    const uint64_t steps = g.W / (4 * static_cast<uint64_t>(S));
    const uint64_t wave = blockIdx.x * (QSV_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (QSV_BLOCK / 64) * RDM_U;
    auto fetch = [&](amp_t (&x)[RDM_U][T], uint64_t q0) {
#pragma unroll
        for (int u = 0; u < RDM_U; ++u) {
            const uint64_t base = deposit(((q0 + u) * 4 + kk) * S + sub, g);
#pragma unroll
            for (int t = 0; t < T; ++t) x[u][t] = __builtin_nontemporal_load(a + base + row_off[t]);
        }
    };
    auto update = [&](const amp_t (&x)[RDM_U][T]) {
        // first halves of every sum, then second halves: 2 C P independent instructions between dependent ones
#pragma unroll
        for (int u = 0; u < RDM_U; ++u) {
            int p = 0;
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = ti; tj < T; ++tj, ++p) {
                    re[u % C][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u][ti].x, x[u][tj].x, re[u % C][p], 0, 0, 0);
                    im[u % C][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u][ti].y, x[u][tj].x, im[u % C][p], 0, 0, 0);
                }
        }
#pragma unroll
        for (int u = 0; u < RDM_U; ++u) {
            int p = 0;
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = ti; tj < T; ++tj, ++p) {
                    re[u % C][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u][ti].y, x[u][tj].y, re[u % C][p], 0, 0, 0);
                    im[u % C][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(-x[u][ti].x, x[u][tj].y, im[u % C][p], 0, 0, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);   // the other buffer's loads stay where they are written: behind these MFMAs
    };
    // A ring of NBUF buffers, no copies between them: while one feeds the matrix cores the loads of the NBUF - 1 others
    // are in flight, and the wait in front of the MFMAs is for the OLDEST buffer only (a register copy at the loop end
    // made the compiler wait for every outstanding load in the middle of the MFMAs: one buffer in flight per wave,
    // 4.3 TB/s).  Every fetch is unconditional (past the end a wave re-reads its first chunk and drops it): with loads
    // under a branch the compiler cannot count how many younger loads are in flight and waits for all of them.
    // T = 4 runs one wave per SIMD (160 accumulator registers) and an update is 40 MFMAs = 1 us: three buffers ahead
    // cover the HBM latency; T = 1 has four waves per SIMD and needs one.
    constexpr int NBUF = T == 1 ? 2 : T == 2 ? 3 : 4;
    amp_t x[NBUF][RDM_U][T];
    const uint64_t first = wave * RDM_U;
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b) {
        const uint64_t q = first + b * stride;
        fetch(x[b], q < steps ? q : first);
    }
    for (uint64_t q0 = first; q0 < steps;) {
#pragma unroll
        for (int b = 0; b < NBUF; ++b) {
            const uint64_t q = q0 + (NBUF - 1) * stride;
            fetch(x[(b + NBUF - 1) % NBUF], q < steps ? q : first);
            update(x[b]);
            q0 += stride;
            if (q0 >= steps) break;
        }
    }
#pragma unroll
    for (int c = 1; c < C; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) {
            re[0][p] += re[c][p];
            im[0][p] += im[c][p];
        }
    // deterministic sum over the four waves of the workgroup, then one partial per workgroup
    for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) {
        if ((threadIdx.x >> 6) == wv) {
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double *slot_re = red + ((p * 2 + 0) * 4 + r) * 64 + lane;
                    double *slot_im = red + ((p * 2 + 1) * 4 + r) * 64 + lane;
                    *slot_re = (wv == 0 ? 0.0 : *slot_re) + re[0][p][r];
                    *slot_im = (wv == 0 ? 0.0 : *slot_im) + im[0][p][r];
                }
        }
        __syncthreads();
    }
    double *out = partials + static_cast<size_t>(blockIdx.x) * (P * 2 * 256);
    for (int e = threadIdx.x; e < P * 2 * 256; e += QSV_BLOCK) out[e] = red[e];
}

// Round 3 form of the same rank update: a WORKGROUP tile staged through LDS, so that HBM is read in whole 1 KiB
// wave-instructions whatever the kept bits are.  k_rdm above lets lane i of the MFMA operand fetch row i itself: the 16
// rows of a group are 2^(kept bit) apart, so with kept bits outside the lowest four every lane touches a different
// 128-byte line (scattered kept bits [0, 5, 12, 25] at n = 28: 2.9 TB/s; k = 6: 1.9).  Here a tile is (16 T rows) x (64
// groups).  A wave-load is 64 CONSECUTIVE amplitudes for one setting c_h of the kept bits >= 6: the lane bits carry the
// kept bits < 6 (rows) and 6 - l free bits (groups); the 16 T loads of a tile (each wave issues 4 T of them, one tile
// ahead, into registers) are written into the LDS tile at [row][group ^ (row & 15)] and read back as MFMA operands --
// lane (i, kk), row tile t, step m reads [16 t + i][(4 m + kk) ^ i]: 16 distinct 16-byte columns per 16-lane group.
// The arithmetic is cut from four to three MFMAs per (tile pair, step): with a = xr_i, b = xi_i, c = xr_j, d = xi_j
//     P1 += a c^T,  P2 += b d^T,  P3 += (a + b)(c - d)^T      re = P1 + P2,   im = b c^T - a d^T = P3 - P1 + P2,
// 7.5 instead of 10 MFMAs per KiB at k = 6 (the kernel that is bound by the matrix cores).  The (pair, step) units of a
// tile are dealt to the four waves: T <= 2: four steps each, all pairs; T = 4: five pairs x eight steps each.
template <int T>
__global__ __launch_bounds__(QSV_BLOCK) __attribute__((amdgpu_waves_per_eu(2, T == 4 ? 2 : 4))) void k_rdm_tile(
    const amp_t *__restrict__ a, const RdmTileArgs g, double *__restrict__ partials) {   // [grid][P][2][256]
    // Work split over the four waves.  T <= 2: four of the sixteen steps each, every tile pair.  T = 4 (ten pairs: all of
    // them would be 240 accumulator registers): five pairs x eight steps.  Both halves run the SAME code on the pair list
    // A = {(0,0), (2,2), (0,1), (2,3), (0,2)} of operand slots; the second half fills slot tt with row tile tt + 1 mod 4
    // and so computes (1,1), (3,3), (1,2), (3,0), (1,3) -- the complement (the cyclic shift maps A onto it), with (3,0)
    // standing for (0,3) as its conjugate transpose (the host reads that block mirrored).  (Two code paths with their
    // own pair lists made the compiler hold both sets of operands: 256 registers and 100 spilled.)
    constexpr int P = T * (T + 1) / 2, NL = 4 * T /* loads per wave and tile */;
    constexpr int MY_P = T == 4 ? 5 : P, MY_M = T == 4 ? 8 : 4;
    constexpr int TILE_BYTES = 16 * T * 64 * 16, RED_BYTES = P * 2 * 256 * 8;
    __shared__ __attribute__((aligned(16))) char smem[TILE_BYTES > RED_BYTES ? TILE_BYTES : RED_BYTES];
    amp_t *tile = reinterpret_cast<amp_t *>(smem);
    double *red = reinterpret_cast<double *>(smem);
    const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    const uint32_t wave_s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // this lane's place in a wave-load: row bits (kept bits < 6) and group bits (the other lane bits)
    uint32_t r_low = 0, f_low = 0;
    {
        int rb = 0, fb = 0;
        for (int b = 0; b < 6; ++b) {
            if ((g.lmask >> b) & 1u) r_low |= ((lane >> b) & 1u) << rb++;
            else f_low |= ((lane >> b) & 1u) << fb++;
        }
    }
    // the NL loads of this wave: load j = NL wave + jj -> c_h = j mod 2^h, block bb = j >> h (s = bb >> l, b = bb mod 2^l).
    // Everything about a load except the lane's own row / group bits is the same for the whole wave: scalar registers.
    const uint32_t per_tile = 1u << (g.l + g.log_s);     // consecutive w values a tile consumes
    auto lds_slot = [&](int jj) {                         // where my amplitude of load jj goes in the tile
        const uint32_t j = NL * wave_s + jj, c_h = j & ((1u << g.h) - 1u), bb = j >> g.h;
        const uint32_t sblk = bb >> g.l, b = bb & ((1u << g.l) - 1u);
        const uint32_t row = (sblk << g.k) | (c_h << g.l) | r_low, slot = (b << (6 - g.l)) | f_low;
        return row * 64 + (slot ^ (row & 15u));
    };
    auto fetch = [&](amp_t (&x)[NL], uint64_t t) {
#pragma unroll
        for (int jj = 0; jj < NL; ++jj) {
            const uint32_t j = NL * wave_s + jj;
            const uint64_t w = t * per_tile + (j >> g.h);
            const uint64_t c_off = g.hoff[j & ((1u << g.h) - 1u)];    // scalar load
            x[jj] = __builtin_nontemporal_load(a + deposit(w << 6, g) + c_off + lane);
        }
    };
    f64x4 p1[MY_P], p2[MY_P], p3[MY_P];
#pragma unroll
    for (int p = 0; p < MY_P; ++p) p1[p] = p2[p] = p3[p] = f64x4{0.0, 0.0, 0.0, 0.0};
    const uint32_t shift = T == 4 ? (wave_s & 1u) : 0u;                       // row-tile rotation of this wave
    const int m_first = MY_M * (T == 4 ? wave_s >> 1 : wave_s);
    // operand slots of pair q (T = 4: the list A above; otherwise every pair ti <= tj in order)
    constexpr int A_I[5] = {0, 2, 0, 2, 0}, A_J[5] = {0, 2, 1, 3, 2};
    amp_t x[NL];
    // tile order: with R regions, the workgroups in flight together read from R places of the register instead of one
    // narrow window per kept-bit setting (kept bits on the top address bits: every stream would sit in the same channels)
    const uint64_t per_region = g.regions > 1 ? g.tiles / g.regions : 0;
    auto place = [&](uint64_t s) { return g.regions > 1 ? (s % g.regions) * per_region + s / g.regions : s; };
    uint64_t t = blockIdx.x;
    fetch(x, place(t));                                   // gridDim.x <= tiles: every workgroup owns at least one
    for (; t < g.tiles; t += gridDim.x) {
#pragma unroll
        for (int jj = 0; jj < NL; ++jj) tile[lds_slot(jj)] = x[jj];
        __syncthreads();
        const uint64_t nxt = t + gridDim.x;
        fetch(x, place(nxt < g.tiles ? nxt : blockIdx.x));   // unconditional (see k_rdm): past the end re-read and drop
        auto step = [&](int mm) {
            const int m = m_first + mm;
            amp_t v[T];
#pragma unroll
            for (int tt = 0; tt < T; ++tt) v[tt] = tile[(16 * ((tt + shift) & (T - 1)) + i) * 64 + ((4 * m + kk) ^ i)];
            if constexpr (T == 4) {
#pragma unroll
                for (int q = 0; q < MY_P; ++q) {
                    const amp_t vi = v[A_I[q]], vj = v[A_J[q]];
                    p1[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi.x, vj.x, p1[q], 0, 0, 0);
                    p2[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi.y, vj.y, p2[q], 0, 0, 0);
                    p3[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi.x + vi.y, vj.x - vj.y, p3[q], 0, 0, 0);
                }
            } else {
                int q = 0;
#pragma unroll
                for (int ti = 0; ti < T; ++ti)
#pragma unroll
                    for (int tj = ti; tj < T; ++tj, ++q) {
                        p1[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].x, v[tj].x, p1[q], 0, 0, 0);
                        p2[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].y, v[tj].y, p2[q], 0, 0, 0);
                        p3[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].x + v[ti].y, v[tj].x - v[tj].y, p3[q], 0, 0, 0);
                    }
            }
            // the next step's LDS reads stay behind these MFMAs: hoisted, the operands of all steps are live at once
            __builtin_amdgcn_sched_barrier(0);
        };
        if constexpr (T == 4) {       // a real loop: unrolled, the eight steps of 15 MFMAs push the allocator into spills
#pragma unroll 1
            for (int mm = 0; mm < MY_M; ++mm) step(mm);
        } else {
#pragma unroll
            for (int mm = 0; mm < MY_M; ++mm) step(mm);
        }
        __syncthreads();                                  // every wave is done with the tile before it is overwritten
    }
    // re = P1 + P2, im = P3 - P1 + P2; deterministic sum over the waves that share a pair, one partial per workgroup.
    // Pair index p of slot pair q: T = 4, first half (0,0) (2,2) (0,1) (2,3) (0,2) = 0 7 1 8 2; second half (1,1) (3,3)
    // (1,2) (3,0) (1,3) = 4 9 5 3 6, where 3 = (0,3) holds the block of (3,0): its conjugate transpose.
    for (uint32_t wv = 0; wv < 4; ++wv) {
        if (wave_s == wv) {
            const bool first = T == 4 ? wv < 2 : wv == 0;
#pragma unroll
            for (int q = 0; q < MY_P; ++q) {
                constexpr int HALF0[5] = {0, 7, 1, 8, 2}, HALF1[5] = {4, 9, 5, 3, 6};
                const int p = T == 4 ? (shift ? HALF1[q] : HALF0[q]) : q;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double *slot_re = red + ((p * 2 + 0) * 4 + r) * 64 + lane;
                    double *slot_im = red + ((p * 2 + 1) * 4 + r) * 64 + lane;
                    *slot_re = (first ? 0.0 : *slot_re) + (p1[q][r] + p2[q][r]);
                    *slot_im = (first ? 0.0 : *slot_im) + (p3[q][r] - p1[q][r] + p2[q][r]);
                }
            }
        }
        __syncthreads();
    }
    double *out = partials + static_cast<size_t>(blockIdx.x) * (P * 2 * 256);
    for (int e = threadIdx.x; e < P * 2 * 256; e += QSV_BLOCK) out[e] = red[e];
}

// out[e] = sum over blocks of partials[block][e].  16 entries x 16 slices per workgroup: slice s adds blocks s, s+16, ...
// in order, the 16 slice sums are added in slice order through LDS -- a fixed summation tree, so the result does not
// depend on scheduling (one thread per entry walking every block took 0.24 ms: a chain of ~1000 dependent-latency loads).
__global__ __launch_bounds__(QSV_BLOCK) void k_sum_partials(const double *__restrict__ partials, int blocks, int entries,
                                                            double *__restrict__ out) {
    __shared__ double part[16][17];
    const int le = threadIdx.x & 15, slice = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + le;
    double s = 0.0;
    if (e < entries)
        for (int b = slice; b < blocks; b += 16) s += partials[static_cast<size_t>(b) * entries + e];
    part[slice][le] = s;
    __syncthreads();
    if (slice == 0 && e < entries) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][le];
        out[e] = t;
    }
}

// Small registers: one thread per entry (i, j) of rho walks every group (2^n amplitudes < 2^14: microseconds).
__global__ __launch_bounds__(QSV_BLOCK) void k_rdm_small(const amp_t *__restrict__ a, const RdmArgs g,
                                                         const uint64_t *__restrict__ hoff, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.D * g.D) return;
    const int i = e / g.D, j = e % g.D;
    double sr = 0.0, si = 0.0;
    for (uint64_t w = 0; w < g.W; ++w) {
        const uint64_t base = deposit(w, g);
        const amp_t x = a[base + hoff[i]], y = a[base + hoff[j]];
        sr += x.x * y.x + x.y * y.y;   // x conj(y)
        si += x.y * y.x - x.x * y.y;
    }
    out[2 * e] = sr;
    out[2 * e + 1] = si;
}

// <a| rho |a> for a ket `a` (2^n amplitudes) and a density matrix stored row-major as a 2n-qubit register:
// partials[2b], [2b+1] = this block's share of sum_ij conj(a_i) rho_ij a_j.  rho is streamed once; the ket stays in L2.
__global__ __launch_bounds__(QSV_BLOCK) void k_expect_density(const amp_t *__restrict__ ket, const amp_t *__restrict__ rho,
                                                              uint64_t dim_bits, double *__restrict__ partials) {
    double re = 0.0, im = 0.0;
    const uint64_t total = 1ull << (2 * dim_bits), mask = (1ull << dim_bits) - 1;
    for (uint64_t e = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const amp_t r = __builtin_nontemporal_load(rho + e);
        const amp_t ai = ket[e >> dim_bits], aj = ket[e & mask];
        // conj(ai) * aj
        const double cr = ai.x * aj.x + ai.y * aj.y, ci = ai.x * aj.y - ai.y * aj.x;
        re += cr * r.x - ci * r.y;
        im += cr * r.y + ci * r.x;
    }
    block_sum2(re, im);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = re;
        partials[2 * blockIdx.x + 1] = im;
    }
}

}  // namespace

// ----------------------------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------------------------
int qsvk_measure_probs(qsv_state *st, int bit, const double e0[4], const double e1[4], double *p0, double *p1) {
    const cplx a{e0[0], e0[1]}, b{e0[2], e0[3]}, c{e1[0], e1[1]}, d{e1[2], e1[3]};
    const dim3 bd(QSV_BLOCK);
    int grid;
    if (streaming_forms(st)) {
        const bool low = bit < QSV_LANE_BITS;
        grid = grid_for(st->amps >> (low ? 0 : 1), QSV_BLOCK * RO_ITEMS, QSV_REDUCE_BLOCKS);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_measure_probs_s<%s>", low ? "true" : "false");
        with_bool(low, [&](auto LOW) {
            hipLaunchKernelGGL(k_measure_probs_s<LOW.value>, dim3(grid), bd, 0, st->stream, st->data, st->amps, bit, a, b, c, d, st->partials);
        });
    } else {
        const uint64_t pairs = st->amps >> 1;
        grid = grid_for(pairs, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_measure_probs");
        hipLaunchKernelGGL(k_measure_probs, dim3(grid), bd, 0, st->stream, st->data, pairs, bit, a, b, c, d, st->partials);
    }
    const int rc = check_launch();
    if (rc) return rc;
    return sum_partials(st, grid, p0, p1);
}

int qsvk_collapse(qsv_state *st, int bit, const double e[4], double scale) {
    const uint64_t pairs = st->amps >> 1;
    const cplx e0{e[0], e[1]}, e1{e[2], e[3]};
    amp_t *fresh = nullptr;
    int rc = qsvk_scratch(st, pairs, &fresh);
    if (rc) return rc;
    const dim3 bd(QSV_BLOCK);
    if (streaming_forms(st)) {
        const bool low = bit < QSV_LANE_BITS;
        const int items = ro_fit_items(ro_move_items(), pairs);
        const dim3 gd(static_cast<unsigned>(pairs / (QSV_BLOCK * items)));
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_collapse_s<%s>", low ? "true" : "false");
        with_bool(low, [&](auto LOW) { with_pow2<1, 4>(items, [&](auto IT) {
            hipLaunchKernelGGL((k_collapse_s<LOW.value, IT.value>), gd, bd, 0, st->stream, st->data, fresh, pairs, bit, e0, e1, scale);
        }); });
    } else {
        const int grid = grid_for(pairs, QSV_BLOCK * 4, 8192);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_collapse");
        hipLaunchKernelGGL(k_collapse, dim3(grid), bd, 0, st->stream, st->data, fresh, pairs, bit, e0, e1, scale);
    }
    rc = check_launch();
    if (rc) return rc;
    st->n -= 1;
    return qsvk_adopt(st, pairs);
}

int qsvk_insert(qsv_state *st, int bit, const double amp[4]) {
    const uint64_t out_amps = st->amps << 1;
    if (!st->owns_data && out_amps > st->capacity)
        return qsv_fail(QSV_ENOMEM, "insert: the caller-owned buffer has no room for one more qubit");
    const cplx a0{amp[0], amp[1]}, a1{amp[2], amp[3]};
    amp_t *fresh = nullptr;
    int rc = qsvk_scratch(st, out_amps, &fresh);
    if (rc) return rc;
    const dim3 bd(QSV_BLOCK);
    if (streaming_forms(st)) {
        const bool low = bit < QSV_LANE_BITS;
        const int items = ro_fit_items(ro_move_items(), st->amps);
        const dim3 gd(static_cast<unsigned>(st->amps / (QSV_BLOCK * items)));
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_insert_s<%s>", low ? "true" : "false");
        with_bool(low, [&](auto LOW) { with_pow2<1, 4>(items, [&](auto IT) {
            hipLaunchKernelGGL((k_insert_s<LOW.value, IT.value>), gd, bd, 0, st->stream, st->data, fresh, st->amps, bit, a0, a1);
        }); });
    } else {
        const int grid = grid_for(out_amps, QSV_BLOCK * 4, 8192);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_insert");
        hipLaunchKernelGGL(k_insert, dim3(grid), bd, 0, st->stream, st->data, fresh, out_amps, bit, a0, a1);
    }
    rc = check_launch();
    if (rc) return rc;
    st->n += 1;
    return qsvk_adopt(st, out_amps);
}

int qsvk_permute(qsv_state *st, const int *src_bit_of_dst_bit) {
    amp_t *fresh = nullptr;
    int rc = qsvk_scratch(st, st->amps, &fresh);
    if (rc) return rc;
    const dim3 bd(QSV_BLOCK);
    if (streaming_forms(st)) {
        const PermTile t = permute_tile(st->n, src_bit_of_dst_bit);
        const size_t bytes = sizeof(uint64_t) * t.lut.size();
        rc = qsvk_ensure_matrix(st, bytes);
        if (rc) return rc;
        QSV_HIP(hipMemcpyAsync(st->dev_matrix, t.lut.data(), bytes, hipMemcpyHostToDevice, st->stream));
        QSV_HIP(hipStreamSynchronize(st->stream));  // the table dies at return
        const int items = ro_move_items();
        const int grid = grid_for(t.args.tiles, (QSV_BLOCK / 64) * items, 1 << 22);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_permute_s");
        with_pow2<1, 4>(items, [&](auto IT) {
            hipLaunchKernelGGL(k_permute_s<IT.value>, dim3(grid), bd, 0, st->stream, st->data, fresh, t.args,
                               reinterpret_cast<const uint64_t *>(st->dev_matrix));
        });
    } else {
        PermArgs g;
        std::memset(&g, 0, sizeof(g));
        g.n = st->n;
        for (int b = 0; b < st->n; ++b) g.src_bit[b] = static_cast<uint8_t>(src_bit_of_dst_bit[b]);
        const int grid = grid_for(st->amps, QSV_BLOCK * 4, 8192);
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_permute");
        hipLaunchKernelGGL(k_permute, dim3(grid), bd, 0, st->stream, st->data, fresh, st->amps, g);
    }
    rc = check_launch();
    if (rc) return rc;
    return qsvk_adopt(st, st->amps);
}

int qsvk_norm2(qsv_state *st, double *out) {
    const int grid = grid_for(st->amps, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_norm2, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, st->partials);
    int rc = check_launch();
    if (rc) return rc;
    return sum_partials(st, grid, out, nullptr);
}

// out[e] = the sum over `blocks` workgroups of partials[block][e], on the device and in a fixed order (k_sum_partials)
int qsvk_sum_partials(hipStream_t stream, const double *partials, int blocks, int entries, double *out) {
    hipLaunchKernelGGL(k_sum_partials, dim3((entries + 15) / 16), dim3(QSV_BLOCK), 0, stream, partials, blocks, entries, out);
    return check_launch();
}

int qsvk_inner(qsv_state *a, qsv_state *b, double *re, double *im) {
    QSV_HIP(hipStreamSynchronize(b->stream));
    const int grid = grid_for(a->amps, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_inner, dim3(grid), dim3(QSV_BLOCK), 0, a->stream, a->data, b->data, a->amps, a->partials);
    int rc = check_launch();
    if (rc) return rc;
    return sum_partials(a, grid, re, im);
}


// rho_out: 4^k complex, row-major, row / column index bit (k-1-j) <-> bits[j] (bits[0] = most significant leg).
int qsvk_reduced_density(qsv_state *st, int k, const int *bits, double *rho_out) {
    if (k < 1 || k > QSV_MAX_K || k > st->n) return qsv_fail(QSV_EINVAL, "reduced density matrix: keep 1..6 qubits");
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, st->device);  // 256 if the query fails
    const RdmPlan p = rdm_plan(st->n, st->amps, k, bits, st->readout_variant, st->remap, cus);
    const size_t b_off = sizeof(uint64_t) * p.off.size(), b_out = sizeof(double) * p.entries,
                 b_part = sizeof(double) * static_cast<size_t>(p.blocks) * p.entries;
    int rc = qsvk_ensure_matrix(st, b_off + b_out + b_part + 64);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(st->dev_matrix);
    uint64_t *d_off = reinterpret_cast<uint64_t *>(base);
    double *d_out = reinterpret_cast<double *>(base + b_off), *d_part = reinterpret_cast<double *>(base + b_off + b_out);
    const bool tile_form = p.big && !p.old_form;
    if (!tile_form) QSV_HIP(hipMemcpyAsync(d_off, p.off.data(), b_off, hipMemcpyHostToDevice, st->stream));
    const dim3 gd(p.blocks), bd(QSV_BLOCK);
    if (p.big) {
        snprintf(st->last_kernel, sizeof(st->last_kernel), tile_form ? "k_rdm_tile<%d>" : "k_rdm<%d>", p.T);
        with_pow2<1, 4>(p.T, [&](auto T) {
            if (tile_form) hipLaunchKernelGGL(k_rdm_tile<T.value>, gd, bd, 0, st->stream, st->data, p.gt, d_part);
            else hipLaunchKernelGGL(k_rdm<T.value>, gd, bd, 0, st->stream, st->data, p.g, d_off, d_part);
        });
        rc = check_launch();
        if (rc && tile_form) return rc;   // no upload of the host's in flight: nothing to wait for
        if (!rc) hipLaunchKernelGGL(k_sum_partials, dim3((p.entries + 15) / 16), bd, 0, st->stream, d_part, p.blocks, p.entries, d_out);
    } else {
        snprintf(st->last_kernel, sizeof(st->last_kernel), "k_rdm_small");
        hipLaunchKernelGGL(k_rdm_small, dim3((p.D * p.D + QSV_BLOCK - 1) / QSV_BLOCK), bd, 0, st->stream, st->data, p.g, d_off, d_out);
    }
    if (!rc) rc = check_launch();
    if (rc) {
        (void)hipStreamSynchronize(st->stream);   // the offsets' upload reads the plan's vector
        return rc;
    }
    std::vector<double> raw(p.entries);
    QSV_HIP(hipMemcpyAsync(raw.data(), d_out, b_out, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    rdm_unpack(p, bits, raw.data(), rho_out);
    return QSV_OK;
}

int qsvk_expect_density(qsv_state *ket, qsv_state *rho, double *re, double *im) {
    QSV_HIP(hipStreamSynchronize(ket->stream));
    const int grid = grid_for(rho->amps, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_expect_density, dim3(grid), dim3(QSV_BLOCK), 0, rho->stream, ket->data, rho->data,
                       static_cast<uint64_t>(ket->n), rho->partials);
    int rc = check_launch();
    if (rc) return rc;
    return sum_partials(rho, grid, re, im);
}

// Inverse-CDF sampling of basis states: out[s] = smallest index i with sum_{j <= i} |amp_j|^2 > u[s] * total.
int qsvk_sample(qsv_state *st, int shots, const double *u, uint64_t *out) {
    const uint64_t chunks = (st->amps + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;
    const size_t sums_bytes = sizeof(double) * chunks, shot_bytes = sizeof(uint64_t) * shots;
    int rc = qsvk_ensure_matrix(st, sums_bytes + 3 * shot_bytes + 64);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(st->dev_matrix);
    double *d_sums = reinterpret_cast<double *>(base);
    uint64_t *d_chunk = reinterpret_cast<uint64_t *>(base + (sums_bytes + 15) / 16 * 16);
    double *d_resid = reinterpret_cast<double *>(d_chunk + shots);
    uint64_t *d_out = reinterpret_cast<uint64_t *>(d_resid + shots);
    hipLaunchKernelGGL(k_chunk_sums, dim3(grid_for(chunks, 1, 1 << 16)), dim3(QSV_BLOCK), 0, st->stream, st->data,
                       st->amps, d_sums);
    rc = check_launch();
    if (rc) return rc;
    std::vector<double> sums(chunks);
    QSV_HIP(hipMemcpyAsync(sums.data(), d_sums, sums_bytes, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    const SampleChunks pick = sample_chunks(sums, u, shots);
    if (pick.status == SampleChunks::ZERO_NORM) return qsv_fail(QSV_EINVAL, "cannot sample from a register of zero norm");
    if (pick.status == SampleChunks::DRAW_OUTSIDE) return qsv_fail(QSV_EINVAL, "uniform draws must lie in [0, 1)");
    QSV_HIP(hipMemcpyAsync(d_chunk, pick.chunk.data(), shot_bytes, hipMemcpyHostToDevice, st->stream));
    QSV_HIP(hipMemcpyAsync(d_resid, pick.resid.data(), sizeof(double) * shots, hipMemcpyHostToDevice, st->stream));
    hipLaunchKernelGGL(k_sample_in_chunk, dim3(shots), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, d_chunk,
                       d_resid, d_out);
    rc = check_launch();
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(out, d_out, shot_bytes, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));  // also covers the two pageable uploads above
    return QSV_OK;
}

int qsvk_probabilities(qsv_state *st, const uint64_t *indices, int count, double *out) {
    if (count <= 0) return QSV_OK;
    const size_t ibytes = sizeof(uint64_t) * count, obytes = sizeof(double) * count;
    int rc = qsvk_ensure_matrix(st, ibytes + obytes);
    if (rc) return rc;
    uint64_t *didx = reinterpret_cast<uint64_t *>(st->dev_matrix);
    double *dout = reinterpret_cast<double *>(reinterpret_cast<char *>(st->dev_matrix) + ibytes);
    QSV_HIP(hipMemcpyAsync(didx, indices, ibytes, hipMemcpyHostToDevice, st->stream));
    hipLaunchKernelGGL(k_gather_prob, dim3((count + 255) / 256), dim3(256), 0, st->stream, st->data, didx, count,
                       dout);
    rc = check_launch();
    if (rc) return rc;
    QSV_HIP(hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    return QSV_OK;
}

int qsvk_fill_random(qsv_state *st, uint64_t seed, uint64_t index_offset, double *norm2) {
    const int grid = grid_for(st->amps, QSV_BLOCK * 8, QSV_REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_fill_random, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, seed,
                       index_offset, st->partials);
    int rc = check_launch();
    if (rc) return rc;
    double s = 0.0;
    rc = sum_partials(st, grid, &s, nullptr);
    if (norm2) *norm2 = s;
    return rc;
}

int qsvk_scale(qsv_state *st, double re, double im) {
    const int grid = grid_for(st->amps, QSV_BLOCK * 8, 8192);
    hipLaunchKernelGGL(k_scale, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, cplx{re, im});
    return check_launch();
}

int qsvk_set_basis(qsv_state *st, uint64_t index) {
    const int grid = grid_for(st->amps, QSV_BLOCK * 8, 8192);
    hipLaunchKernelGGL(k_zero, dim3(grid), dim3(QSV_BLOCK), 0, st->stream, st->data, st->amps, index);
    return check_launch();
}

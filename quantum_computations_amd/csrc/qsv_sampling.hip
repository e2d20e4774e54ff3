// Multi-shot homodyne sampling of a matrix-product state: one site step for a block of shots (SiteRegister.sample).
//
// Every shot s carries a boundary vector V[s, :] of length L, the chain to its left collapsed onto the shot's earlier
// outcomes.  For the site A (L x d x R, row-major) the step is
//     w[s, j, b]  = sum_a V[s, a] A[a, j, b]                                  (never stored)
//     p[s, j]     = sum_b |w[s, j, b]|^2                 or, with the right environment E folded into AE = A . E,
//                 = Re sum_b conj(w[s, j, b]) wE[s, j, b]     with wE = V . AE  (the diagonal of partial_density_mps,
//                                                                                mps.py:176-190, for the collapsed chain)
//     pick[s]     = first j with cumsum(p[s, :])[j] / cumsum(p[s, :])[d - 1] > u[s]      (rng.choice of gates.py:98)
//     density[s]  = scale * p[s, pick[s]]                                                (gates.py:102)
//     V'[s, :]    = V[s, :] . A[:, pick[s], :] / sqrt(density[s])                        (gates.py:108-113)
//
// k_sample_weights is the hot path: 8 S L d R real flops (twice that with an environment) on v_mfma_f64_16x16x4_f64.
// For one grid point j the product is D (R x S) = A_j^T (R x L) . V^T (L x S): the MFMA's A operand is
// A[a = 4q + (lane >> 4), j, b = 16 bt + (lane & 15)] -- one 16-byte global load per lane, 256 contiguous bytes per
// 16-lane group -- and its B operand V[s = 16 st + (lane & 15), a], read from an LDS image of the workgroup's 16 ST shots
// that is loaded once and used for every (j, b) of the workgroup.  A complex product is four real MFMAs (as in
// k_skinny_nn).  D has the shot on the lane (col = lane & 15) and b on the rows (row = (lane >> 4) + 4 reg), so squaring
// and summing over b is four multiply-adds per lane per tile, carried across the b tiles in registers, and two
// cross-lane adds per grid point at the end.  Each loaded element of A feeds 4 ST MFMAs: at ST = 4 (64 shots) that is
// 32 flop per byte of A.  The order of every sum is fixed by (L, R) alone, so equal inputs give equal bits whatever
// the number of shots or the block they fall in.
//
// k_sample_pick: one wave per shot scans the d weights twice in 64-wide steps (first for the total, then for the first
// CDF value above u), then the same wave advances the shot's boundary vector.
//
// Self-contained: no other translation unit refers to a symbol of this file.  The p workspace (shots x d doubles, in
// blocks of at most 256 MiB) comes from the grow-only pool of the (device, stream) context; the call ends with a
// synchronisation of its stream, as the pool's contract requires.
#include <cmath>

#include "qsv_linalg.h"

using namespace qsvl;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr size_t P_BLOCK_BYTES = 256ull << 20;     // upper bound of the p workspace
constexpr size_t LDS_LIMIT = 128ull << 10;         // V image of one workgroup (the CU has 160 KiB)

// P[s, j] for the shots of blockIdx.x (16 ST of them) and the grid points of blockIdx.y's chunk; wave w of the
// workgroup takes the points j = chunk_begin + w, + 4, ...  Lq = ceil(L / 4) MFMA steps; V rows past L are zero.
template <int ST, bool ENV>
__global__ __launch_bounds__(256) void k_sample_weights(const amp_t *__restrict__ V, const amp_t *__restrict__ A,
                                                       const amp_t *__restrict__ AE, double *__restrict__ P, uint64_t S,
                                                       uint64_t L, uint64_t d, uint64_t R, unsigned Lq, unsigned j_chunk) {
    extern __shared__ amp_t vs[];                      // [4 Lq][16 ST]
    constexpr int SB = 16 * ST;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const uint64_t s0 = static_cast<uint64_t>(blockIdx.x) * SB;
    const unsigned Lpad = 4 * Lq;
    // lanes run along a (rows of V are contiguous in a)
    for (unsigned e = t; e < Lpad * SB; e += 256) {
        const unsigned a = e % Lpad, s = e / Lpad;
        amp_t v = amp_t{0.0, 0.0};
        if (a < L && s0 + s < S) v = V[(s0 + s) * L + a];
        vs[a * SB + s] = v;
    }
    __syncthreads();

    const uint64_t j_begin = static_cast<uint64_t>(blockIdx.y) * j_chunk;
    const uint64_t j_end = j_begin + j_chunk < d ? j_begin + j_chunk : d;
    const unsigned b_tiles = static_cast<unsigned>((R + 15) / 16);
    for (uint64_t j = j_begin + wave; j < j_end; j += 4) {
        double part[ST];
#pragma unroll
        for (int st = 0; st < ST; ++st) part[st] = 0.0;
        for (unsigned bt = 0; bt < b_tiles; ++bt) {
            const uint64_t b = 16ull * bt + li;
            const bool b_ok = b < R;
            f64x4 wre[ST], wim[ST], ere[ENV ? ST : 1], eim[ENV ? ST : 1];
#pragma unroll
            for (int st = 0; st < ST; ++st) wre[st] = wim[st] = f64x4{0.0, 0.0, 0.0, 0.0};
            if (ENV) {
#pragma unroll
                for (int st = 0; st < ST; ++st) ere[st] = eim[st] = f64x4{0.0, 0.0, 0.0, 0.0};
            }
            for (unsigned q = 0; q < Lq; ++q) {
                const uint64_t a = 4ull * q + lk;
                const bool ok = b_ok && a < L;
                const uint64_t at = (a * d + j) * R + b;
                const amp_t x = ok ? A[at] : amp_t{0.0, 0.0};
                amp_t xe = amp_t{0.0, 0.0};
                if (ENV && ok) xe = AE[at];
                amp_t v[ST];
#pragma unroll
                for (int st = 0; st < ST; ++st) v[st] = vs[static_cast<unsigned>(a) * SB + 16 * st + li];
#pragma unroll
                for (int st = 0; st < ST; ++st) {       // dependent updates of one accumulator stay apart
                    wre[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, v[st].x, wre[st], 0, 0, 0);
                    wim[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, v[st].y, wim[st], 0, 0, 0);
                }
#pragma unroll
                for (int st = 0; st < ST; ++st) {
                    wre[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(-x.y, v[st].y, wre[st], 0, 0, 0);
                    wim[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.y, v[st].x, wim[st], 0, 0, 0);
                }
                if (ENV) {
#pragma unroll
                    for (int st = 0; st < ST; ++st) {
                        ere[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(xe.x, v[st].x, ere[st], 0, 0, 0);
                        eim[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(xe.x, v[st].y, eim[st], 0, 0, 0);
                    }
#pragma unroll
                    for (int st = 0; st < ST; ++st) {
                        ere[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xe.y, v[st].y, ere[st], 0, 0, 0);
                        eim[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(xe.y, v[st].x, eim[st], 0, 0, 0);
                    }
                }
            }
            // rows of D are b (zero past R), the column is the shot: square and sum the lane's four rows
#pragma unroll
            for (int st = 0; st < ST; ++st)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    if (ENV) part[st] += wre[st][reg] * ere[st][reg] + wim[st][reg] * eim[st][reg];
                    else part[st] += wre[st][reg] * wre[st][reg] + wim[st][reg] * wim[st][reg];
                }
        }
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            double sum = part[st];
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const uint64_t s = s0 + 16 * st + li;
            if (lk == 0 && s < S) P[s * d + j] = sum;
        }
    }
}

// One wave per shot: pick, density and the advanced boundary vector (V_out may be null: the last site has none).
__global__ __launch_bounds__(256) void k_sample_pick(const double *__restrict__ P, const double *__restrict__ u,
                                                    const amp_t *__restrict__ V, const amp_t *__restrict__ A, uint64_t S,
                                                    uint64_t L, uint64_t d, uint64_t R, double scale,
                                                    int32_t *__restrict__ pick, double *__restrict__ density,
                                                    amp_t *__restrict__ V_out) {
    const int lane = threadIdx.x & 63;
    const uint64_t shot = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (shot >= S) return;                               // whole waves leave; no barrier below
    const double *p = P + shot * d;
    // inclusive scan in 64-wide steps; the same arithmetic in both passes, so the last CDF value is exactly 1
    auto scan_step = [&](uint64_t base, double carry) {
        double x = base + lane < d ? p[base + lane] : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        return carry + x;
    };
    double carry = 0.0;
    for (uint64_t base = 0; base < d; base += 64) carry = __shfl(scan_step(base, carry), 63, 64);
    const double total = carry, threshold = u[shot];
    uint64_t chosen = d - 1;
    carry = 0.0;
    for (uint64_t base = 0; base < d; base += 64) {
        const double cum = scan_step(base, carry);
        const bool hit = base + lane < d && cum / total > threshold;
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            chosen = base + static_cast<uint64_t>(__builtin_ctzll(mask));
            break;
        }
        carry = __shfl(cum, 63, 64);
    }
    const double rho = scale * p[chosen];
    if (lane == 0) {
        pick[shot] = static_cast<int32_t>(chosen);
        density[shot] = rho;
    }
    if (!V_out) return;
    const double root = sqrt(rho);
    const amp_t *v = V + shot * L;
    for (uint64_t b = lane; b < R; b += 64) {
        double re = 0.0, im = 0.0;
        for (uint64_t a = 0; a < L; ++a) {
            const amp_t x = A[(a * d + chosen) * R + b], c = v[a];
            re += c.x * x.x - c.y * x.y;
            im += c.x * x.y + c.y * x.x;
        }
        V_out[shot * R + b] = amp_t{re / root, im / root};
    }
}

template <int ST>
int launch_weights(hipStream_t stream, const amp_t *V, const amp_t *A, const amp_t *AE, double *P, uint64_t S, uint64_t L,
                   uint64_t d, uint64_t R) {
    const unsigned Lq = static_cast<unsigned>((L + 3) / 4);
    const size_t lds = static_cast<size_t>(4) * Lq * 16 * ST * sizeof(amp_t);
    const uint64_t blocks = (S + 16 * ST - 1) / (16 * ST);
    // enough workgroups to fill the device when there are few shots, at least four grid points (one per wave) each
    uint64_t chunks = (2048 + blocks - 1) / blocks;
    const uint64_t most = (d + 3) / 4;
    if (chunks > most) chunks = most;
    if (chunks > 65535) chunks = 65535;
    if (chunks < 1) chunks = 1;
    const unsigned j_chunk = static_cast<unsigned>((d + chunks - 1) / chunks);
    const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>((d + j_chunk - 1) / j_chunk));
    auto go = [&](auto kernel) -> int {
        if (lds > (64u << 10))
            QSV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)));
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, V, A, AE, P, S, L, d, R, Lq, j_chunk);
        QSV_HIP(hipGetLastError());
        return QSV_OK;
    };
    return AE ? go(k_sample_weights<ST, true>) : go(k_sample_weights<ST, false>);
}

}  // namespace

int qsv_tensor_sample_site(int device, void *hip_stream, const void *dev_v, const void *dev_site, const void *dev_site_env,
                           uint64_t S, uint64_t L, uint64_t d, uint64_t R, double scale, const double *dev_u,
                           int32_t *dev_pick, double *dev_density, void *dev_v_out) {
    // every check before the first HIP call
    if (!dev_v || !dev_site || !dev_u || !dev_pick || !dev_density) return qsv_fail(QSV_EINVAL, "null pointer");
    if (device < 0 || device >= 16) return qsv_fail(QSV_EINVAL, "device index out of range");
    if (S < 1) return qsv_fail(QSV_EINVAL, "sampling needs at least one shot");
    if (d < 2) return qsv_fail(QSV_EINVAL, "sampling needs a grid of at least two points");
    if (L < 1 || R < 1) return qsv_fail(QSV_EINVAL, "empty bond");
    if (d > 0x7fffffffull) return qsv_fail(QSV_EINVAL, "grid too large");
    if (S > (1ull << 40)) return qsv_fail(QSV_EINVAL, "too many shots for one call");
    if (R > (1ull << 20)) return qsv_fail(QSV_EINVAL, "right bond too large");
    if (!(scale > 0.0) || !std::isfinite(scale)) return qsv_fail(QSV_EINVAL, "scale must be positive and finite");
    // the boundary vectors of a workgroup's shots live in LDS: 64 shots up to bond 128, 32 up to 256, 16 up to 512
    const uint64_t Lpad = (L + 3) / 4 * 4;
    const int shot_tiles = Lpad * 64 * sizeof(amp_t) <= LDS_LIMIT ? 4 : Lpad * 32 * sizeof(amp_t) <= LDS_LIMIT ? 2 : 1;
    if (Lpad * 16 * shot_tiles * sizeof(amp_t) > LDS_LIMIT)
        return qsv_fail(QSV_EINVAL, "left bond " + std::to_string(L) + " exceeds the sampling kernel's limit of 512");

    uint64_t block = P_BLOCK_BYTES / (d * 8);
    block = block >= 64 ? block / 64 * 64 : 64;          // whole workgroups of shots, except in the last block
    if (block > S) block = S;
    if ((block + 63) / 64 * 4 > 0x7fffffffull) return qsv_fail(QSV_EINVAL, "shot block too large for one launch");

    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc;
    StreamContext *ctx = context_for(device, stream, &rc);
    if (!ctx) return rc;
    DeviceBuffers buf;
    const size_t bytes_p = block * d * 8;
    buf.reserve(*ctx, (bytes_p + 255) / 256 * 256);
    double *P;
    if (!buf.alloc(&P, bytes_p)) return qsv_fail(QSV_ENOMEM, "sampling workspace allocation failed");

    const amp_t *V = static_cast<const amp_t *>(dev_v), *A = static_cast<const amp_t *>(dev_site);
    const amp_t *AE = static_cast<const amp_t *>(dev_site_env);
    amp_t *V_out = static_cast<amp_t *>(dev_v_out);
    for (uint64_t s0 = 0; s0 < S; s0 += block) {
        const uint64_t n = S - s0 < block ? S - s0 : block;
        const amp_t *Vb = V + s0 * L;
        rc = shot_tiles == 4   ? launch_weights<4>(stream, Vb, A, AE, P, n, L, d, R)
             : shot_tiles == 2 ? launch_weights<2>(stream, Vb, A, AE, P, n, L, d, R)
                               : launch_weights<1>(stream, Vb, A, AE, P, n, L, d, R);
        if (rc != QSV_OK) return rc;
        hipLaunchKernelGGL(k_sample_pick, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0, stream, P, dev_u + s0, Vb, A,
                           n, L, d, R, scale, dev_pick + s0, dev_density + s0, V_out ? V_out + s0 * R : nullptr);
        QSV_HIP(hipGetLastError());
    }
    QSV_HIP(hipStreamSynchronize(stream));      // the pool is free again only when the kernels are done
    return QSV_OK;
}

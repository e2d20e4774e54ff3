// Tall-skinny products of the range finder on the f64 matrix cores: skinny_gemm (for qsv_rsvd.hip) and qsvg_skinny_gemm.
//
//   k_skinny_nn :  Y (n x l) = A (n x m) . Q (m x l)          k_skinny_cn :  Y (m x l) = A^H (m x n) . Q (n x l)
//
// A is the big operand (column-major, ld n: gigabytes), Q / Y are panels of l <= 64 columns.  rocBLAS pads such panels
// to a 64-wide macro tile and streams A at 2.2 TB/s whatever l is; these kernels tile l in steps of 16
// (v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D col = lane & 15,
// row = (lane >> 4) + 4 reg), stage the Q slab through LDS once per workgroup and keep A as one 16-byte load per lane
// per k-step.  A complex product is four real MFMAs; one wave owns 16 rows (nn) or 16 columns (cn) of A.
// The sum over k may be taken in any order as long as both operands use the same one: the cn kernel lets a lane
// fetch two consecutive rows (32 contiguous bytes) and spends them on two successive MFMA steps, so that the four lane
// groups cover whole 128-byte lines of every column.
#include "qsv_linalg.h"

using namespace qsvl;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int SK_SLAB = qsv_split_rules::SKINNY_SLAB;           // k values per LDS slab of Q

template <int T>                      // T = number of 16-column tiles of the panel (l <= 16 T)
__global__ __launch_bounds__(256) void k_skinny_nn(const amp_t *__restrict__ A, const amp_t *__restrict__ Q,
                                                  amp_t *__restrict__ Y, uint64_t n, uint64_t m, int l,
                                                  double im_sign, amp_t *__restrict__ shares) {
    __shared__ amp_t slab[2][SK_SLAB][16 * T + 1];   // +1: the column-wise slab stores would otherwise hit one bank
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * 64 + wave * 16 + li;
    const bool row_ok = row < n;
    f64x4 cre[T], cim[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cre[j] = cim[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const uint64_t all_slabs = (m + SK_SLAB - 1) / SK_SLAB;
    // split-K: blockIdx.y takes a contiguous share of the slabs; with two shares the two partial sums meet in a
    // zero-initialised Y through atomic adds, and a + b does not depend on which arrives first
    const uint64_t s_begin = all_slabs * blockIdx.y / gridDim.y, slabs = all_slabs * (blockIdx.y + 1) / gridDim.y;
    constexpr int QREGS = SK_SLAB * 16 * T / 256;     // slab entries per thread
    amp_t q_next[QREGS];
    auto load_q = [&](uint64_t s) {              // Q[k0 + k][j] of slab s -> registers, zero padded
        const uint64_t k0 = s * SK_SLAB;
#pragma unroll
        for (int u = 0; u < QREGS; ++u) {
            const int e = t + 256 * u, k = e % SK_SLAB, j = e / SK_SLAB;
            q_next[u] = (k0 + k < m && j < l) ? Q[static_cast<uint64_t>(j) * m + k0 + k] : amp_t{0.0, 0.0};
        }
    };
    auto store_q = [&](int buf) {
#pragma unroll
        for (int u = 0; u < QREGS; ++u) {
            const int e = t + 256 * u;
            slab[buf][e % SK_SLAB][e / SK_SLAB] = q_next[u];
        }
    };
    amp_t a_now[SK_SLAB / 4], a_next[SK_SLAB / 4];
    auto fetch = [&](amp_t *dst, uint64_t s) {
        const uint64_t k0 = s * SK_SLAB;
#pragma unroll
        for (int q = 0; q < SK_SLAB / 4; ++q) {
            const uint64_t k = k0 + 4 * q + lk;
            dst[q] = (row_ok && k < m) ? __builtin_nontemporal_load(A + k * n + row) : amp_t{0.0, 0.0};
        }
    };
    load_q(s_begin);
    store_q(s_begin & 1);
    fetch(a_now, s_begin);
    for (uint64_t s = s_begin; s < slabs; ++s) {
        const int buf = s & 1;
        __syncthreads();                               // slab[buf] is complete, slab[buf ^ 1] is free
        const bool more = s + 1 < slabs;
        if (more) {                                    // loads for the next slab fly while this one is multiplied
            load_q(s + 1);
            fetch(a_next, s + 1);
        }
#pragma unroll
        for (int q = 0; q < SK_SLAB / 4; ++q) {
            const double are = a_now[q].x, aim = im_sign * a_now[q].y;   // im_sign = -1: conj(A) Q
            amp_t b[T];
#pragma unroll
            for (int j = 0; j < T; ++j) b[j] = slab[buf][4 * q + lk][16 * j + li];
#pragma unroll
            for (int j = 0; j < T; ++j) {        // dependent updates of one accumulator stay 2 T instructions apart
                cre[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, b[j].x, cre[j], 0, 0, 0);
                cim[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, b[j].y, cim[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < T; ++j) {
                cre[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, b[j].y, cre[j], 0, 0, 0);
                cim[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, b[j].x, cim[j], 0, 0, 0);
            }
        }
        if (more) {
            store_q(buf ^ 1);
#pragma unroll
            for (int q = 0; q < SK_SLAB / 4; ++q) a_now[q] = a_next[q];
        }
    }
    // D: col = lane & 15, row = (lane >> 4) + 4 reg
    const uint64_t row_base = static_cast<uint64_t>(blockIdx.x) * 64 + wave * 16;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int col = 16 * j + li;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint64_t r = row_base + lk + 4 * reg;
            if (r < n && col < l) {
                amp_t *dst = Y + static_cast<uint64_t>(col) * n + r;
                if (gridDim.y == 1) {
                    *dst = amp_t{cre[j][reg], cim[j][reg]};
                } else if (shares) {        // k_sum_shares adds the shares in order
                    shares[(static_cast<uint64_t>(blockIdx.y) * l + col) * n + r] = amp_t{cre[j][reg], cim[j][reg]};
                } else {
                    atomicAdd(reinterpret_cast<double *>(dst), cre[j][reg]);
                    atomicAdd(reinterpret_cast<double *>(dst) + 1, cim[j][reg]);
                }
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(256) void k_skinny_cn(const amp_t *__restrict__ A, const amp_t *__restrict__ Q,
                                                  amp_t *__restrict__ Y, uint64_t n, uint64_t m, int l,
                                                  double im_sign, amp_t *__restrict__ shares) {
    __shared__ amp_t slab[2][SK_SLAB][16 * T + 1];   // +1: the column-wise slab stores would otherwise hit one bank
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const uint64_t col = static_cast<uint64_t>(blockIdx.x) * 64 + wave * 16 + li;   // column of A = output row
    const bool col_ok = col < m;
    f64x4 cre[T], cim[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cre[j] = cim[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const uint64_t all_slabs = (n + SK_SLAB - 1) / SK_SLAB;
    const uint64_t s_begin = all_slabs * blockIdx.y / gridDim.y, slabs = all_slabs * (blockIdx.y + 1) / gridDim.y;
    constexpr int QREGS = SK_SLAB * 16 * T / 256;
    amp_t q_next[QREGS];
    auto load_q = [&](uint64_t s) {              // Q[r0 + k][j] of slab s -> registers
        const uint64_t r0 = s * SK_SLAB;
#pragma unroll
        for (int u = 0; u < QREGS; ++u) {
            const int e = t + 256 * u, k = e % SK_SLAB, j = e / SK_SLAB;
            q_next[u] = (r0 + k < n && j < l) ? Q[static_cast<uint64_t>(j) * n + r0 + k] : amp_t{0.0, 0.0};
        }
    };
    auto store_q = [&](int buf) {
#pragma unroll
        for (int u = 0; u < QREGS; ++u) {
            const int e = t + 256 * u;
            slab[buf][e % SK_SLAB][e / SK_SLAB] = q_next[u];
        }
    };
    // rows of a slab in blocks of 8: lane group lk owns rows 8 b + 2 lk and 8 b + 2 lk + 1 (32 contiguous bytes)
    amp_t a_now[SK_SLAB / 4], a_next[SK_SLAB / 4];
    auto fetch = [&](amp_t *dst, uint64_t s) {
        const uint64_t r0 = s * SK_SLAB;
#pragma unroll
        for (int b = 0; b < SK_SLAB / 8; ++b)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint64_t r = r0 + 8 * b + 2 * lk + h;
                dst[2 * b + h] = (col_ok && r < n) ? __builtin_nontemporal_load(A + col * n + r) : amp_t{0.0, 0.0};
            }
    };
    load_q(s_begin);
    store_q(s_begin & 1);
    fetch(a_now, s_begin);
    for (uint64_t s = s_begin; s < slabs; ++s) {
        const int buf = s & 1;
        __syncthreads();
        const bool more = s + 1 < slabs;
        if (more) {
            load_q(s + 1);
            fetch(a_next, s + 1);
        }
#pragma unroll
        for (int b = 0; b < SK_SLAB / 8; ++b)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // the MFMAs below take conj(A): (are, -aim); im_sign = -1 turns that into the plain transpose
                const double are = a_now[2 * b + h].x, aim = im_sign * a_now[2 * b + h].y;
                amp_t q[T];
#pragma unroll
                for (int j = 0; j < T; ++j) q[j] = slab[buf][8 * b + 2 * lk + h][16 * j + li];
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    cre[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, q[j].x, cre[j], 0, 0, 0);
                    cim[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, q[j].y, cim[j], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    cre[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, q[j].y, cre[j], 0, 0, 0);
                    cim[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, q[j].x, cim[j], 0, 0, 0);
                }
            }
        if (more) {
            store_q(buf ^ 1);
#pragma unroll
            for (int q = 0; q < SK_SLAB / 4; ++q) a_now[q] = a_next[q];
        }
    }
    const uint64_t out_base = static_cast<uint64_t>(blockIdx.x) * 64 + wave * 16;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int pc = 16 * j + li;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint64_t r = out_base + lk + 4 * reg;
            if (r < m && pc < l) {
                amp_t *dst = Y + static_cast<uint64_t>(pc) * m + r;
                if (gridDim.y == 1) {
                    *dst = amp_t{cre[j][reg], cim[j][reg]};
                } else if (shares) {
                    shares[(static_cast<uint64_t>(blockIdx.y) * l + pc) * m + r] = amp_t{cre[j][reg], cim[j][reg]};
                } else {
                    atomicAdd(reinterpret_cast<double *>(dst), cre[j][reg]);
                    atomicAdd(reinterpret_cast<double *>(dst) + 1, cim[j][reg]);
                }
            }
        }
    }
}

// Y[i] = shares[0][i] + shares[1][i] + ... in that order (the k ranges of a split-K skinny product)
__global__ __launch_bounds__(256) void k_sum_shares(const amp_t *__restrict__ shares, amp_t *__restrict__ Y, uint64_t count,
                                                   int n_shares) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= count) return;
    amp_t v[SKINNY_MAX_SHARES];
#pragma unroll
    for (int s = 0; s < static_cast<int>(SKINNY_MAX_SHARES); ++s)
        if (s < n_shares) v[s] = shares[static_cast<uint64_t>(s) * count + i];
    amp_t sum = v[0];
#pragma unroll
    for (int s = 1; s < static_cast<int>(SKINNY_MAX_SHARES); ++s)
        if (s < n_shares) {
            sum.x += v[s].x;
            sum.y += v[s].y;
        }
    Y[i] = sum;
}

}  // namespace

bool qsvl::skinny_gemm(hipStream_t stream, bool transpose, bool conjugate, const amp_t *A, const amp_t *Q, amp_t *Y,
                       uint64_t n, uint64_t m, int l, amp_t *shares, uint64_t share_amps) {
    if (l < 1 || l > WIDE_MAX) return false;
    const uint64_t out_rows = transpose ? m : n;
    if (l > 64) {        // panels wider than the kernels' 64 columns: one pass over A per 64-column slice
        const uint64_t q_rows = transpose ? n : m;
        for (int c0 = 0; c0 < l; c0 += 64)
            if (!skinny_gemm(stream, transpose, conjugate, A, Q + static_cast<uint64_t>(c0) * q_rows,
                             Y + static_cast<uint64_t>(c0) * out_rows, n, m, l - c0 < 64 ? l - c0 : 64, shares, share_amps))
                return false;
        return true;
    }
    const int tiles = (l + 15) / 16;
    const unsigned row_blocks = static_cast<unsigned>((out_rows + 63) / 64);
    const auto [split, shared_out] = qsv_split_rules::skinny_share_plan(out_rows, transpose ? n : m, l, shares ? share_amps : 0);
    if (split > 1 && !shared_out && hipMemsetAsync(Y, 0, sizeof(amp_t) * out_rows * l, stream) != hipSuccess) return false;
    const dim3 grid(row_blocks, split), block(256);
    amp_t *share_arg = shared_out ? shares : nullptr;
    // k_skinny_nn multiplies by (re, im_sign * im); k_skinny_cn by the conjugate of that
    const double im_sign = transpose ? (conjugate ? 1.0 : -1.0) : (conjugate ? -1.0 : 1.0);
#define QSV_SKINNY(T)                                                                                                    \
    if (transpose) hipLaunchKernelGGL(k_skinny_cn<T>, grid, block, 0, stream, A, Q, Y, n, m, l, im_sign, share_arg);     \
    else hipLaunchKernelGGL(k_skinny_nn<T>, grid, block, 0, stream, A, Q, Y, n, m, l, im_sign, share_arg)
    switch (tiles) {
        case 1: QSV_SKINNY(1); break;
        case 2: QSV_SKINNY(2); break;
        case 3: QSV_SKINNY(3); break;
        default: QSV_SKINNY(4); break;
    }
#undef QSV_SKINNY
    if (shared_out) {
        const uint64_t count = out_rows * l;
        hipLaunchKernelGGL(k_sum_shares, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, shares, Y,
                           count, static_cast<int>(split));
    }
    return hipGetLastError() == hipSuccess;
}

// Column-major tall-skinny product on the f64 matrix cores (see k_skinny_nn / k_skinny_cn).
int qsvg_skinny_gemm(int device, hipStream_t stream, int op, uint64_t n, uint64_t m, int l, const amp_t *A,
                     const amp_t *Q, amp_t *Y) {
    QSV_HIP(hipSetDevice(device));
    // op: 0 = A, 1 = A^H, 2 = A^T, 3 = conj(A)
    if (!skinny_gemm(stream, op == 1 || op == 2, op == 1 || op == 3, A, Q, Y, n, m, l))
        return qsv_fail(QSV_EINVAL, "panel width must be 1..256 columns");
    return QSV_OK;
}

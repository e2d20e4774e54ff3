// Internal: the rocBLAS / rocSOLVER binding and the per-stream contexts (handle, scratch pool) used by qsv_gemm.hip (plain
// GEMMs), qsv_phase_space.hip, qsv_canonical.hip and the MPS splits, whose files also find here what crosses between them:
//   qsv_decomp.hip  the exact split (qsvg_svd_split) and the Jacobi sweeps over a whole matrix
//   qsv_rsvd.hip    the randomized split (qsvg_rsvd_split), the verified low-rank route, the library-QR fallback
//   qsv_panel.hip   CholeskyQR3 panels, block Gram-Schmidt beyond 64 columns, the Jacobi SVDs of the small factors
//   qsv_skinny.hip  the tall-skinny MFMA products (qsvg_skinny_gemm)
// (qsv_split_rules.h: their host-side decisions; qsv_jacobi.h: the Jacobi step of their kernels.)  Both libraries are
// bound with dlopen on first use: libqsv.so keeps loading -- and the qubit path keeps working -- on a machine without
// them, and inside a PyTorch process the copies PyTorch already loaded are reused.
#pragma once

#include <cstdint>
#include <mutex>
#include <vector>

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "qsv_internal.h"
#include "qsv_split_rules.h"

namespace qsvl {

struct RocblasApi {
    decltype(&rocblas_create_handle) create = nullptr;
    decltype(&rocblas_destroy_handle) destroy = nullptr;
    decltype(&rocblas_set_stream) set_stream = nullptr;
    decltype(&rocblas_zgemm_strided_batched) zgemm = nullptr;
    decltype(&rocsolver_zgesvd) zgesvd = nullptr;      // null when rocSOLVER is absent: SVD entry points fail loudly
    decltype(&rocsolver_zgesdd) zgesdd = nullptr;
    decltype(&rocsolver_zgeqrf) zgeqrf = nullptr;
    decltype(&rocsolver_zungqr) zungqr = nullptr;
    bool ok = false;
    std::once_flag once;  // the libraries are bound once; afterwards the table is read-only
};

RocblasApi &api();
bool loaded(RocblasApi &a);
rocblas_operation op_of(int op);

// Scratch memory of the decompositions: a grow-only pool per stream context (a split needs a copy of theta plus panels --
// gigabytes -- and hipMalloc / hipFree of that size on every call costs milliseconds, and hipFree waits for the whole
// device).  A pool that grows keeps its old block in `retired` until the context is released: growing frees nothing.
struct Pool {
    char *base = nullptr;
    size_t capacity = 0;
};

// Everything a tensor call on one (device, stream) mutates: its own rocBLAS handle (bound to the stream once), its own
// scratch pool, the partial sums of the low-rank route and the memo of the ask-for-omega protocol of qsvg_rsvd_split.
// Calls on one stream come from one thread at a time (include/qsv.h), so a context is never used by two calls at once
// and needs no lock of its own; only the map that holds the contexts has one, taken for lookup and insertion.
struct StreamContext {
    int device = 0;
    hipStream_t stream = nullptr;
    rocblas_handle handle = nullptr;   // created on first use: the Wigner path needs the pool but not rocBLAS
    Pool pool;
    std::vector<char *> retired;       // outgrown pool blocks, freed with the context
    double *norm_partials = nullptr;   // 256 doubles, see try_verified_low_rank
    const void *asked_theta = nullptr; // qsvg_rsvd_split: the theta a caller was asked to bring its test matrix for
    uint64_t asked_rows = 0, asked_cols = 0;
};

// The context of (device, stream), created on first use; null (and *rc set) for a bad device ordinal.
StreamContext *context_for(int device, hipStream_t stream, int *rc);
// The context's rocBLAS handle, or null (and *rc set) when the libraries cannot be used.
rocblas_handle handle_of(StreamContext &ctx, int *rc);
// Make the pool of `ctx` at least `bytes` large.  Growth allocates a new block and retires the old one (no hipFree, so
// no wait for the device).  QSV_OK or an error.
int reserve_pool(StreamContext &ctx, size_t bytes);

// A DeviceBuffers object carves from the pool of one context; requests the pool cannot hold fall back to hipMalloc and
// are freed when the object goes out of scope.  Calls end with a synchronisation of their stream, so the pool is free
// again when the next call on the same stream starts.
struct DeviceBuffers {
    Pool *pool = nullptr;
    size_t used = 0;
    void *extra[12] = {};
    int n = 0;

    // Make the pool of `ctx` at least `bytes` large (no-op when it already is).  Call before the first alloc.  When the
    // pool cannot grow, allocations fall back to hipMalloc.
    void reserve(StreamContext &ctx, size_t bytes) {
        (void)reserve_pool(ctx, bytes);
        pool = &ctx.pool;
    }

    template <class T>
    bool alloc(T **out, size_t bytes) {
        const size_t need = (bytes + 255) / 256 * 256;
        if (pool && pool->base && used + need <= pool->capacity) {
            *out = reinterpret_cast<T *>(pool->base + used);
            used += need;
            return true;
        }
        if (n >= 12 || hipMalloc(reinterpret_cast<void **>(out), bytes ? bytes : 16) != hipSuccess) return false;
        extra[n++] = *out;
        return true;
    }

    ~DeviceBuffers() {
        for (int i = 0; i < n; ++i) (void)hipFree(extra[i]);
    }
};

// ---- between the files of the MPS splits ------------------------------------------------------------------------------
constexpr int LMAX = 64;             // widest panel the fused kernels take
constexpr int WIDE_MAX = 256;        // widest panel the blocked (64-column) forms take
constexpr int GRAM_BLOCKS = 64;      // partial Gram matrices per panel (summed by one workgroup: keep it short)
constexpr int QSV_UNDECIDED = 2;     // a route declines: the next one decides (theta is untouched)
using qsv_split_rules::SKINNY_MAX_SHARES;

inline int blocks_for(uint64_t items) {
    const uint64_t b = (items + QSV_BLOCK - 1) / QSV_BLOCK;
    return static_cast<int>(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

inline const rocblas_double_complex *Z(const amp_t *p) { return reinterpret_cast<const rocblas_double_complex *>(p); }
inline rocblas_double_complex *Z(amp_t *p) { return reinterpret_cast<rocblas_double_complex *>(p); }
// C (M x N) = op(A) op(B) with K summed, column-major; false when rocBLAS reports a failure
inline bool zgemm(RocblasApi &a, rocblas_handle h, rocblas_operation ta, rocblas_operation tb, rocblas_int M, rocblas_int N,
                  rocblas_int K, const amp_t *pa, rocblas_int lda, const amp_t *pb, rocblas_int ldb, amp_t *pc, rocblas_int ldc) {
    const rocblas_double_complex one{1.0, 0.0}, zero{0.0, 0.0};
    return a.zgemm(h, ta, tb, M, N, K, &one, Z(pa), lda, 0, Z(pb), ldb, 0, &zero, Z(pc), ldc, 0, 1) == rocblas_status_success;
}

// qsv_skinny.hip.  Y = op(A) Q with A (n x m), everything column-major with tight leading dimensions:
//   transpose == false: Y (n x l) = A Q or conj(A) Q   (Q is m x l);   transpose == true: Y (m x l) = A^T Q or A^H Q   (Q is n x l).
// Returns false when the shape is outside what the kernels take (l > WIDE_MAX) so that the caller can use the library instead.
// `shares` (optional, room for `share_amps` amplitudes): workspace that lets a product with few output rows cut its k
// range into up to 16 shares (one workgroup each, summed in order by k_sum_shares) instead of two
bool skinny_gemm(hipStream_t stream, bool transpose, bool conjugate, const amp_t *A, const amp_t *Q, amp_t *Y, uint64_t n,
                 uint64_t m, int l, amp_t *shares = nullptr, uint64_t share_amps = 0);
// qsv_panel.hip.  Orthonormalise a column-major (n x l) panel, l <= WIDE_MAX, in place; `r_total` (l x l row-major, may be
// null) receives the factor with Y_in = Y_out * r_total.  `partials`: GRAM_BLOCKS * min(l, LMAX)^2 amplitudes, `scratch`:
// 2 * LMAX * LMAX, `flags`: 4 ints.
int wide_panel_orthonormalise(hipStream_t stream, amp_t *Y, uint64_t n, int l, amp_t *partials, amp_t *scratch, amp_t *r_total,
                              int *flags, int rounds = 3);
// qsv_panel.hip.  R = U_r S V_r^H for the row-major l x l triangle R, l <= WIDE_MAX, by one-sided Jacobi; U_r, V_r
// column-major, S sorted decreasingly.  `work`: 2 l^2 amplitudes (used beyond LMAX), `flag`: one device int.
int factor_svd(hipStream_t stream, const amp_t *R, int l, amp_t *work, amp_t *Ur, double *S, amp_t *Vr, int *flag);
// qsv_rsvd.hip.  The exact split's shortcut for a numerically low-rank theta: QSV_OK with the split in (m1, m2, *rank_out)
// and the first s_count values of the spectrum (zeros beyond the computed ones) in s_host (may be null), QSV_UNDECIDED
// when the rank cannot be verified, or an error.
int try_verified_low_rank(RocblasApi &a, rocblas_handle h, StreamContext &ctx, const amp_t *theta, uint64_t rows, uint64_t cols,
                          int64_t max_bond_dim, double abs_err, double rel_err, amp_t *m1, amp_t *m2, uint64_t capacity,
                          uint64_t *rank_out, double *s_host, uint64_t s_count, double *frobenius_squared_out = nullptr);

}  // namespace qsvl

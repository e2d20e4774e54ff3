// Internal: the rocBLAS / rocSOLVER binding and the per-stream contexts (handle, scratch pool) used by qsv_gemm.hip (plain
// GEMMs), qsv_decomp.hip (splits, panel kernels) and qsv_phase_space.hip.  Both libraries are bound with dlopen on first
// use: libqsv.so keeps loading -- and the qubit path keeps working -- on a machine without them, and inside a PyTorch
// process the copies PyTorch already loaded are reused.
#pragma once

#include <cstdint>
#include <mutex>
#include <vector>

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "qsv_internal.h"

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

}  // namespace qsvl

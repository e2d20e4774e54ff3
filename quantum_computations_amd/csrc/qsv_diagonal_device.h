// What the translation units that read a device diagonal share (qsv_diagonal.hip, which makes and owns it, and qsv_sweep.hip,
// which applies one diagonal to every member of an ensemble): the object itself and the device functions of the phase
// kernels, so that a member's cost phase rounds exactly as a register's of its own does.  Everything here is static; no
// __global__ function lives here.
#pragma once

#include "qsv_device.h"
#include "qsv_diagonal_layout.h"

struct qsv_diag {
    int device = 0;
    int n = 0;
    uint64_t size = 1;               // 2^n doubles at `data`
    double *data = nullptr;
    hipStream_t stream = nullptr;
    int grid_cap = 0;
    qsv_diagonal_layout::DiagTerm *table = nullptr;       // device copy of the term table of the last qsv_diag_set_pauli_sum
    size_t table_rows = 0;           // rows allocated
    uint64_t *scratch = nullptr;     // partials of k_diag_extrema
    size_t scratch_bytes = 0;
    char last_kernel[96] = "";
};

template <bool NT>
static __device__ __forceinline__ double ld_real(const double *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// exp(-i gamma x): one double-precision sincos
static __device__ __forceinline__ cplx phase_of(double gamma, double x) {
    double s, c;
    sincos(gamma * x, &s, &c);
    return cplx{c, -s};
}

// The diagonal's own work is finished before a kernel on another stream reads it.
static int wait_for_diag(const qsv_diag *d, hipStream_t launching) {
    if (d->stream != launching) QSV_HIP(hipStreamSynchronize(d->stream));
    return QSV_OK;
}

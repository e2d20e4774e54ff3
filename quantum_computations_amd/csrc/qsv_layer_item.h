// The one statement of a product layer's arithmetic: what a stage does to the pair (a, b) of amplitudes with the stage's
// index bit 0 / 1.  Included by every kernel form of qsv_layer.hip, so that where a stage sits -- tile pass, run, the form
// below one tile, member of an ensemble -- never changes its bits.  Device functions only, static.
#pragma once

#include "qsv_device.h"

struct LayerMatrix {
    cplx m00, m01, m10, m11;
};

// eight doubles, row-major interleaved complex (the table's and the C ABI's order)
static __device__ __forceinline__ LayerMatrix layer_matrix(const double *m) {
    return LayerMatrix{cplx{m[0], m[1]}, cplx{m[2], m[3]}, cplx{m[4], m[5]}, cplx{m[6], m[7]}};
}

static __device__ __forceinline__ void layer_item(amp_t &a, amp_t &b, const LayerMatrix &m) {
    const amp_t lo = cfma(m.m01, b, cmul(m.m00, a));
    const amp_t hi = cfma(m.m11, b, cmul(m.m10, a));
    a = lo;
    b = hi;
}

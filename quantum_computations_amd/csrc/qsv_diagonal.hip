// Real diagonal operators held on the device (gfx950, wave64) and their C entry points: qsv_diag is
// a vector of 2^n doubles indexed like the register; qsv_diag_set_pauli_sum builds it from any number of Z-only terms in
// ONE write pass; qsv_apply_diag_phase / _mul, qsv_expect_diag, qsv_diag_transition and qsv_diag_phase_adjoint are one pass
// over the register each.  Pure streaming kernels: one 16-byte access per amplitude and one 8-byte load of the diagonal
// per lane, no LDS except in the reductions.  Term packing, grids and the slices of the scratch buffer come from
// qsv_diagonal_layout.h.

#include "qsv_device.h"
#include "qsv_diagonal_device.h"

#include <cstring>
#include <limits>
#include <vector>

using namespace qsv_diagonal_layout;

static_assert(DIAG_BLOCK == QSV_BLOCK && DIAG_REDUCE_BLOCKS == QSV_REDUCE_BLOCKS, "qsv_diagonal_layout.h mirrors qsv_internal.h");

namespace {

// qsv_diag itself, ld_real, phase_of and wait_for_diag: qsv_diagonal_device.h, shared with qsv_sweep.hip.

// d[i] = (ACC ? d[i] : 0) + sum_t coeff_t (-1)^popcount(i & zmask_t), the additions in table order, one rounded add per
// term: coeff * (+-1) is a flip of the sign bit.  The table index is wave-uniform and the table is never written by the
// kernel, so its rows arrive through the scalar data path (one four-dword scalar load per row and wave), and the loop
// costs a popcount, a shift, an xor and an add per element and term.
template <bool ACC>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_build(double *__restrict__ d, uint64_t size, const DiagTerm *__restrict__ table,
                                                          uint32_t n_terms) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < size; i += stride) {
        double acc = 0.0;
        if constexpr (ACC) acc = d[i];
#pragma unroll 4   // four rows requested together; the additions stay in table order
        for (uint32_t t = 0; t < n_terms; ++t) {
            const DiagTerm row = table[t];
            const uint64_t flip = static_cast<uint64_t>(__popcll(i & row.zmask) & 1) << 63;
            acc += __longlong_as_double(static_cast<long long>(static_cast<uint64_t>(__double_as_longlong(row.coeff)) ^ flip));
        }
        d[i] = acc;
    }
}

// psi[i] *= exp(-i gamma d[i])
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_phase(amp_t *__restrict__ psi, const double *__restrict__ d, uint64_t amps, double gamma) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < amps; i += stride) {
        const amp_t a = ld<NT>(psi + i);
        const double x = ld_real<NT>(d + i);
        st<NT>(psi + i, cmul(phase_of(gamma, x), a));
    }
}

// dst[i] = (ACC ? dst[i] : 0) + c d[i] src[i].  Without ACC the old dst is never read (NaN in it does not spread) and dst
// may be src: every thread loads its amplitude before it stores it.  No __restrict__ on dst / src for that reason.
template <bool ACC, bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_mul(amp_t *dst, const amp_t *src, const double *__restrict__ d, uint64_t amps,
                                                        double c_re, double c_im) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < amps; i += stride) {
        const amp_t s = ld<NT>(src + i);
        const double x = ld_real<NT>(d + i);
        const cplx m = {c_re * x, c_im * x};
        amp_t out;
        if constexpr (ACC)
            out = cfma(m, s, ld<NT>(dst + i));
        else
            out = cmul(m, s);
        st<NT>(dst + i, out);
    }
}

// The workgroup's sums of K doubles per thread -> partials[block * K + k]: wave shuffle, LDS, one partial per slot.
template <int K>
__device__ __forceinline__ void block_store_sums(const double (&v)[K], double *__restrict__ partials) {
    __shared__ double sums[QSV_BLOCK / 64][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = 0.0;
        for (int wv = 0; wv < QSV_BLOCK / 64; ++wv) s += sums[wv][threadIdx.x];
        partials[static_cast<uint64_t>(blockIdx.x) * K + threadIdx.x] = s;
    }
}

// partials[block][4] = this workgroup's share of { sum p, sum p d, sum p d^2, sum_{d <= threshold} p }, p = |psi|^2.
// THR = false: no threshold, slot 3 is 0.  Read-only.
template <bool THR>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_expect(const amp_t *__restrict__ psi, const double *__restrict__ d, uint64_t amps,
                                                           double threshold, double *__restrict__ partials) {
    double v[EXPECT_SLOTS] = {0.0, 0.0, 0.0, 0.0};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < amps; i += stride) {
        const amp_t a = psi[i];
        const double x = d[i];
        const double p = fma(a.x, a.x, a.y * a.y);
        const double px = p * x;
        v[0] += p;
        v[1] += px;
        v[2] = fma(px, x, v[2]);
        if constexpr (THR) v[3] += x <= threshold ? p : 0.0;
    }
    block_store_sums<EXPECT_SLOTS>(v, partials);
}

// conj(x) y
__device__ __forceinline__ amp_t conj_mul(amp_t x, amp_t y) {
    return amp_t{fma(x.x, y.x, x.y * y.y), fma(x.x, y.y, -(x.y * y.x))};
}

// partials[block][2] = this workgroup's share of <bra|D ket> = sum_i conj(bra[i]) d[i] ket[i].  Read-only; bra may be ket.
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_transition(const amp_t *bra, const amp_t *ket, const double *__restrict__ d,
                                                               uint64_t amps, double *__restrict__ partials) {
    double v[TRANSITION_SLOTS] = {0.0, 0.0};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < amps; i += stride) {
        const amp_t p = conj_mul(bra[i], ket[i]);
        const double x = d[i];
        v[0] = fma(p.x, x, v[0]);
        v[1] = fma(p.y, x, v[1]);
    }
    block_store_sums<TRANSITION_SLOTS>(v, partials);
}

// The diagonal counterpart of k_pauli_adjoint_group: partials[block][2] = share of <lambda|D psi>, then both registers
// take the phase exp(-i gamma d).  D commutes with the phase, so the value is the same before and after it; one sincos
// per amplitude serves both registers.
template <bool NT>
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_phase_adjoint(amp_t *__restrict__ psi, amp_t *__restrict__ lambda, const double *__restrict__ d,
                                                                  uint64_t amps, double gamma, double *__restrict__ partials) {
    double v[TRANSITION_SLOTS] = {0.0, 0.0};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < amps; i += stride) {
        const amp_t a = ld<NT>(psi + i), l = ld<NT>(lambda + i);
        const double x = ld_real<NT>(d + i);
        const amp_t p = conj_mul(l, a);
        v[0] = fma(p.x, x, v[0]);
        v[1] = fma(p.y, x, v[1]);
        const cplx ph = phase_of(gamma, x);
        st<NT>(psi + i, cmul(ph, a));
        st<NT>(lambda + i, cmul(ph, l));
    }
    block_store_sums<TRANSITION_SLOTS>(v, partials);
}

// partials[block][4] = { min, argmin, max, argmax } of this workgroup's elements as 8-byte words; ties go to the lowest
// index.  A thread's indices grow, so strict comparisons keep its first; lanes and waves are combined on (value, index).
__global__ __launch_bounds__(QSV_BLOCK) void k_diag_extrema(const double *__restrict__ d, uint64_t size, uint64_t *__restrict__ partials) {
    double mn = __builtin_inf(), mx = -__builtin_inf();
    unsigned long long amn = ~0ull, amx = ~0ull;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * QSV_BLOCK;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(QSV_BLOCK) + threadIdx.x; i < size; i += stride) {
        const double x = d[i];
        if (x < mn || amn == ~0ull) {
            mn = x;
            amn = i;
        }
        if (x > mx || amx == ~0ull) {
            mx = x;
            amx = i;
        }
    }
    auto take_min = [&](double v, unsigned long long a) {
        if (a != ~0ull && (amn == ~0ull || v < mn || (v == mn && a < amn))) {
            mn = v;
            amn = a;
        }
    };
    auto take_max = [&](double v, unsigned long long a) {
        if (a != ~0ull && (amx == ~0ull || v > mx || (v == mx && a < amx))) {
            mx = v;
            amx = a;
        }
    };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v0 = __shfl_xor(mn, o, 64), v1 = __shfl_xor(mx, o, 64);
        const unsigned long long a0 = __shfl_xor(amn, o, 64), a1 = __shfl_xor(amx, o, 64);
        take_min(v0, a0);
        take_max(v1, a1);
    }
    __shared__ double s_mn[QSV_BLOCK / 64], s_mx[QSV_BLOCK / 64];
    __shared__ unsigned long long s_amn[QSV_BLOCK / 64], s_amx[QSV_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        s_mn[threadIdx.x >> 6] = mn;
        s_mx[threadIdx.x >> 6] = mx;
        s_amn[threadIdx.x >> 6] = amn;
        s_amx[threadIdx.x >> 6] = amx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < QSV_BLOCK / 64; ++wv) {
            take_min(s_mn[wv], s_amn[wv]);
            take_max(s_mx[wv], s_amx[wv]);
        }
        uint64_t *out = partials + static_cast<uint64_t>(blockIdx.x) * EXTREMA_SLOTS;
        out[0] = static_cast<uint64_t>(__double_as_longlong(mn));
        out[1] = amn;
        out[2] = static_cast<uint64_t>(__double_as_longlong(mx));
        out[3] = amx;
    }
}

int check_diag(const qsv_diag *d) { return d ? QSV_OK : qsv_fail(QSV_EINVAL, "null diagonal"); }

// A register and a diagonal that can meet in one pass.
int check_pair(const qsv_state *st, const qsv_diag *d) {
    if (st->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    if (st->device != d->device) return qsv_fail(QSV_EINVAL, "register and diagonal on different devices");
    if (st->n != d->n || st->amps != d->size) return qsv_fail(QSV_EINVAL, "register and diagonal of different sizes");
    return QSV_OK;
}

// One copy and one synchronisation on st's stream; out[slot] = the partials summed in index order.
int fetch_sums(qsv_state *st, const ReducePlan &plan, double *out) {
    std::vector<double> host(plan.words);
    QSV_HIP(hipMemcpyAsync(host.data(), st->dev_matrix, plan.bytes, hipMemcpyDeviceToHost, st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    reduce_sums(plan, host.data(), out);
    return QSV_OK;
}

bool ranges_meet(const amp_t *a, const amp_t *b, uint64_t amps) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + sizeof(amp_t) * amps && b0 < a0 + sizeof(amp_t) * amps;
}

}  // namespace

extern "C" {

int qsv_diag_create(int n_qubits, int device, qsv_diag **out) {
    if (!out) return qsv_fail(QSV_EINVAL, "null pointer");
    *out = nullptr;
    if (n_qubits < 0 || n_qubits > 40) return qsv_fail(QSV_EINVAL, "n_qubits must be in 0..40");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return qsv_fail(QSV_EHIP, "no HIP device");
    if (device < 0 || device >= count) return qsv_fail(QSV_EINVAL, "no such device");
    QSV_HIP(hipSetDevice(device));
    qsv_diag *d = new qsv_diag;
    d->device = device;
    d->n = n_qubits;
    d->size = 1ull << n_qubits;
    if (hipMalloc(reinterpret_cast<void **>(&d->data), sizeof(double) * d->size) != hipSuccess) {
        delete d;
        return qsv_fail(QSV_ENOMEM, "device allocation of the diagonal failed");
    }
    hipError_t e = hipMemsetAsync(d->data, 0, sizeof(double) * d->size, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) {
        (void)hipFree(d->data);
        delete d;
        return qsv_fail(QSV_EHIP, std::string("zero-fill of the diagonal: ") + hipGetErrorString(e));
    }
    *out = d;
    return QSV_OK;
}

int qsv_diag_destroy(qsv_diag *d) {
    if (!d) return QSV_OK;
    (void)hipSetDevice(d->device);
    (void)hipStreamSynchronize(d->stream);
    if (d->data) (void)hipFree(d->data);
    if (d->table) (void)hipFree(d->table);
    if (d->scratch) (void)hipFree(d->scratch);
    delete d;
    return QSV_OK;
}

int qsv_diag_set_stream(qsv_diag *d, void *hip_stream) {
    if (check_diag(d)) return QSV_EINVAL;
    QSV_HIP(hipSetDevice(d->device));
    QSV_HIP(hipStreamSynchronize(d->stream));
    d->stream = static_cast<hipStream_t>(hip_stream);
    return QSV_OK;
}

int qsv_diag_num_qubits(const qsv_diag *d, int *n_qubits) {
    if (!d || !n_qubits) return qsv_fail(QSV_EINVAL, "null pointer");
    *n_qubits = d->n;
    return QSV_OK;
}

int qsv_diag_set_option(qsv_diag *d, int option, int64_t value) {
    if (check_diag(d)) return QSV_EINVAL;
    if (option != QSV_OPT_GRID_CAP) return qsv_fail(QSV_EINVAL, "a diagonal has the grid-cap option only");
    if (value < 0 || value > (1 << 30)) return qsv_fail(QSV_EINVAL, "bad grid cap");
    d->grid_cap = static_cast<int>(value);
    return QSV_OK;
}

int qsv_diag_last_kernel(const qsv_diag *d, char *buf, size_t buf_len) {
    if (!d || !buf || buf_len == 0) return qsv_fail(QSV_EINVAL, "null pointer");
    strncpy(buf, d->last_kernel, buf_len - 1);
    buf[buf_len - 1] = '\0';
    return QSV_OK;
}

int qsv_diag_upload(qsv_diag *d, const double *host, uint64_t offset, uint64_t count) {
    if (!d || (!host && count)) return qsv_fail(QSV_EINVAL, "null pointer");
    if (offset > d->size || count > d->size - offset) return qsv_fail(QSV_EINVAL, "upload range out of bounds");
    if (count == 0) return QSV_OK;
    QSV_HIP(hipSetDevice(d->device));
    QSV_HIP(hipMemcpyAsync(d->data + offset, host, sizeof(double) * count, hipMemcpyHostToDevice, d->stream));
    QSV_HIP(hipStreamSynchronize(d->stream));
    return QSV_OK;
}

int qsv_diag_download(qsv_diag *d, double *host, uint64_t offset, uint64_t count) {
    if (!d || (!host && count)) return qsv_fail(QSV_EINVAL, "null pointer");
    if (offset > d->size || count > d->size - offset) return qsv_fail(QSV_EINVAL, "download range out of bounds");
    if (count == 0) return QSV_OK;
    QSV_HIP(hipSetDevice(d->device));
    QSV_HIP(hipMemcpyAsync(host, d->data + offset, sizeof(double) * count, hipMemcpyDeviceToHost, d->stream));
    QSV_HIP(hipStreamSynchronize(d->stream));
    return QSV_OK;
}

int qsv_diag_set_pauli_sum(qsv_diag *d, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                           const double *coeffs, int accumulate, uint64_t *passes) {
    if (check_diag(d)) return QSV_EINVAL;
    if (n_terms < 0) return qsv_fail(QSV_EINVAL, "negative number of terms");
    std::vector<DiagTerm> rows;
    const PackError bad = pack_terms(d->n, n_terms, term_offsets, qubits, paulis, coeffs, &rows);
    if (bad != PACK_OK) return qsv_fail(QSV_EINVAL, pack_error_text(bad));
    if (passes) *passes = 0;
    if (rows.empty() && accumulate) return QSV_OK;
    QSV_HIP(hipSetDevice(d->device));
    if (rows.size() > d->table_rows) {
        if (d->table) {
            QSV_HIP(hipStreamSynchronize(d->stream));
            QSV_HIP(hipFree(d->table));
            d->table = nullptr;
            d->table_rows = 0;
        }
        const size_t want = std::max<size_t>(rows.size(), 64);
        if (hipMalloc(reinterpret_cast<void **>(&d->table), sizeof(DiagTerm) * want) != hipSuccess)
            return qsv_fail(QSV_ENOMEM, "device allocation of the term table failed");
        d->table_rows = want;
    }
    if (!rows.empty()) {
        // the rows die with this call: the copy is finished before it returns (one synchronisation per build)
        QSV_HIP(hipMemcpyAsync(d->table, rows.data(), sizeof(DiagTerm) * rows.size(), hipMemcpyHostToDevice, d->stream));
        QSV_HIP(hipStreamSynchronize(d->stream));
    }
    const dim3 gd(stream_grid(d->size, d->grid_cap)), bd(QSV_BLOCK);
    const uint32_t count = static_cast<uint32_t>(rows.size());
    with_bool(accumulate != 0, [&](auto ACC) {
        hipLaunchKernelGGL((k_diag_build<ACC.value>), gd, bd, 0, d->stream, d->data, d->size, static_cast<const DiagTerm *>(d->table), count);
    });
    snprintf(d->last_kernel, sizeof(d->last_kernel), "k_diag_build<%s>", accumulate ? "true" : "false");
    const int rc = check_launch();
    if (rc) return rc;
    if (passes) *passes = 1;
    return QSV_OK;
}

int qsv_diag_extrema(qsv_diag *d, double *min, uint64_t *argmin, double *max, uint64_t *argmax) {
    if (check_diag(d)) return QSV_EINVAL;
    QSV_HIP(hipSetDevice(d->device));
    const ReducePlan plan = reduce_plan(d->size, d->grid_cap, EXTREMA_SLOTS);
    if (d->scratch_bytes < plan.bytes) {
        if (d->scratch) {
            QSV_HIP(hipStreamSynchronize(d->stream));
            QSV_HIP(hipFree(d->scratch));
            d->scratch = nullptr;
            d->scratch_bytes = 0;
        }
        const size_t want = reduce_plan(d->size, 0, EXTREMA_SLOTS).bytes;      // whatever the cap becomes later
        if (hipMalloc(reinterpret_cast<void **>(&d->scratch), want) != hipSuccess)
            return qsv_fail(QSV_ENOMEM, "device allocation of the reduction scratch failed");
        d->scratch_bytes = want;
    }
    hipLaunchKernelGGL(k_diag_extrema, dim3(plan.grid), dim3(QSV_BLOCK), 0, d->stream, static_cast<const double *>(d->data), d->size, d->scratch);
    snprintf(d->last_kernel, sizeof(d->last_kernel), "k_diag_extrema");
    const int rc = check_launch();
    if (rc) return rc;
    std::vector<uint64_t> host(plan.words);
    QSV_HIP(hipMemcpyAsync(host.data(), d->scratch, plan.bytes, hipMemcpyDeviceToHost, d->stream));
    QSV_HIP(hipStreamSynchronize(d->stream));
    const Extrema e = reduce_extrema(plan, host.data());
    if (min) *min = e.min;
    if (argmin) *argmin = e.argmin;
    if (max) *max = e.max;
    if (argmax) *argmax = e.argmax;
    return QSV_OK;
}

int qsv_apply_diag_phase(qsv_state *st, qsv_diag *d, double gamma) {
    if (!st || !d) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_pair(st, d);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = wait_for_diag(d, st->stream);
    if (rc) return rc;
    const bool nt = st->nontemporal != 0;
    const dim3 gd(stream_grid(st->amps, st->grid_cap)), bd(QSV_BLOCK);
    with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_diag_phase<NT.value>), gd, bd, 0, st->stream, st->data, static_cast<const double *>(d->data), st->amps, gamma);
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag_phase<%s>", nt ? "true" : "false");
    return check_launch();
}

int qsv_apply_diag_mul(qsv_state *dst, qsv_state *src, qsv_diag *d, double c_re, double c_im, int accumulate) {
    if (!dst || !src || !d) return qsv_fail(QSV_EINVAL, "null pointer");
    if (dst->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    int rc = check_pair(src, d);
    if (rc) return rc;
    if (dst->device != src->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    if (dst->capacity < src->amps) return qsv_fail(QSV_ENOMEM, "destination register too small");
    if (accumulate && dst->n != src->n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    const bool same = dst == src || dst->data == src->data;
    if (same && accumulate) return qsv_fail(QSV_EINVAL, "the destination of an accumulating call must not be the source");
    if (!same && ranges_meet(dst->data, src->data, src->amps))
        return qsv_fail(QSV_EINVAL, "the destination must not share part of its memory with the source");
    rc = qsv_flush(dst);
    if (rc) return rc;
    rc = qsv_flush(src);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(dst->device));
    if (src->stream != dst->stream) QSV_HIP(hipStreamSynchronize(src->stream));
    rc = wait_for_diag(d, dst->stream);
    if (rc) return rc;
    const bool nt = dst->nontemporal != 0;
    const dim3 gd(stream_grid(src->amps, dst->grid_cap)), bd(QSV_BLOCK);
    with_bool(accumulate != 0, [&](auto ACC) { with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_diag_mul<ACC.value, NT.value>), gd, bd, 0, dst->stream, dst->data, static_cast<const amp_t *>(src->data),
                           static_cast<const double *>(d->data), src->amps, c_re, c_im);
    }); });
    snprintf(dst->last_kernel, sizeof(dst->last_kernel), "k_diag_mul<%s, %s>", accumulate ? "true" : "false", nt ? "true" : "false");
    rc = check_launch();
    if (rc) return rc;
    dst->n = src->n;
    dst->amps = src->amps;
    return QSV_OK;
}

int qsv_expect_diag(qsv_state *st, qsv_diag *d, const double *threshold, double *out) {
    if (!st || !d || !out) return qsv_fail(QSV_EINVAL, "null pointer");
    int rc = check_pair(st, d);
    if (rc) return rc;
    rc = qsv_flush(st);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(st->device));
    rc = wait_for_diag(d, st->stream);
    if (rc) return rc;
    const ReducePlan plan = reduce_plan(st->amps, st->grid_cap, EXPECT_SLOTS);
    rc = qsvk_ensure_matrix(st, plan.bytes);
    if (rc) return rc;
    const double thr = threshold ? *threshold : 0.0;
    with_bool(threshold != nullptr, [&](auto THR) {
        hipLaunchKernelGGL((k_diag_expect<THR.value>), dim3(plan.grid), dim3(QSV_BLOCK), 0, st->stream, static_cast<const amp_t *>(st->data),
                           static_cast<const double *>(d->data), st->amps, thr, st->dev_matrix);
    });
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_diag_expect<%s>", threshold ? "true" : "false");
    rc = check_launch();
    if (rc) return rc;
    return fetch_sums(st, plan, out);
}

int qsv_diag_transition(qsv_state *bra, qsv_state *ket, qsv_diag *d, double *re, double *im) {
    if (!bra || !ket || !d || !re || !im) return qsv_fail(QSV_EINVAL, "null pointer");
    if (bra->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    int rc = check_pair(ket, d);
    if (rc) return rc;
    if (bra->device != ket->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    if (bra->n != ket->n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    rc = qsv_flush(bra);
    if (rc) return rc;
    rc = qsv_flush(ket);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(bra->device));
    if (ket->stream != bra->stream) QSV_HIP(hipStreamSynchronize(ket->stream));
    rc = wait_for_diag(d, bra->stream);
    if (rc) return rc;
    const ReducePlan plan = reduce_plan(bra->amps, bra->grid_cap, TRANSITION_SLOTS);
    rc = qsvk_ensure_matrix(bra, plan.bytes);
    if (rc) return rc;
    hipLaunchKernelGGL(k_diag_transition, dim3(plan.grid), dim3(QSV_BLOCK), 0, bra->stream, static_cast<const amp_t *>(bra->data),
                       static_cast<const amp_t *>(ket->data), static_cast<const double *>(d->data), bra->amps, bra->dev_matrix);
    snprintf(bra->last_kernel, sizeof(bra->last_kernel), "k_diag_transition");
    rc = check_launch();
    if (rc) return rc;
    double sums[TRANSITION_SLOTS];
    rc = fetch_sums(bra, plan, sums);
    if (rc) return rc;
    *re = sums[0];
    *im = sums[1];
    return QSV_OK;
}

int qsv_diag_phase_adjoint(qsv_state *psi, qsv_state *lambda, qsv_diag *d, double gamma, double *re, double *im) {
    if (!psi || !lambda || !d || !re || !im) return qsv_fail(QSV_EINVAL, "null pointer");
    if (lambda->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs qubit registers");
    int rc = check_pair(psi, d);
    if (rc) return rc;
    if (lambda->device != psi->device) return qsv_fail(QSV_EINVAL, "registers on different devices");
    if (lambda->n != psi->n) return qsv_fail(QSV_EINVAL, "registers of different sizes");
    if (lambda == psi || ranges_meet(psi->data, lambda->data, psi->amps))
        return qsv_fail(QSV_EINVAL, "psi and lambda must be two registers whose memory does not meet");
    rc = qsv_flush(psi);
    if (rc) return rc;
    rc = qsv_flush(lambda);
    if (rc) return rc;
    QSV_HIP(hipSetDevice(psi->device));
    if (lambda->stream != psi->stream) QSV_HIP(hipStreamSynchronize(lambda->stream));
    rc = wait_for_diag(d, psi->stream);
    if (rc) return rc;
    const ReducePlan plan = reduce_plan(psi->amps, psi->grid_cap, TRANSITION_SLOTS);
    rc = qsvk_ensure_matrix(psi, plan.bytes);
    if (rc) return rc;
    const bool nt = psi->nontemporal != 0;
    with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_diag_phase_adjoint<NT.value>), dim3(plan.grid), dim3(QSV_BLOCK), 0, psi->stream, psi->data, lambda->data,
                           static_cast<const double *>(d->data), psi->amps, gamma, psi->dev_matrix);
    });
    snprintf(psi->last_kernel, sizeof(psi->last_kernel), "k_diag_phase_adjoint<%s>", nt ? "true" : "false");
    rc = check_launch();
    if (rc) return rc;
    // the copy waits for the kernel on psi's stream: both registers are finished when the call returns
    double sums[TRANSITION_SLOTS];
    rc = fetch_sums(psi, plan, sums);
    if (rc) return rc;
    *re = sums[0];
    *im = sums[1];
    return QSV_OK;
}

}  // extern "C"

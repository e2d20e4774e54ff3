// Device and host helpers shared by the qubit-register translation units of libqsv.so (the gate families qsv_gate12.hip,
// qsv_gatek.hip, qsv_sequence.hip and qsv_pass.hip, qsv_state.hip: staging ring / spare buffer / copy, qsv_readout.hip:
// measurement / reshaping / reductions, qsv_pauli.hip: Pauli sums and rotations).  Everything here is static: each
// translation unit compiles its own copy.  No __global__ function lives here: a kernel is defined in exactly one .hip file.
#pragma once

#include "qsv_internal.h"

#include <cstdlib>
#include <string>
#include <type_traits>

// the accumulator of v_mfma_f64_16x16x4_f64 (k_dense_mfma, k_dense_mtile5, k_rdm, k_rdm_tile)
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct cplx {
    double re, im;
};

static __device__ __forceinline__ amp_t cmul(cplx m, amp_t a) {
    amp_t r;
    r.x = m.re * a.x - m.im * a.y;
    r.y = m.re * a.y + m.im * a.x;
    return r;
}

// d * a for the diagonal kernels (k_diag, and k_pass_tile's diagonal gates), with the two fused multiply-adds spelled
// out: left to the compiler, `re * a.y + im * a.x` is contracted one way or the other depending on the surrounding code,
// and a deferred gate must round exactly as its per-gate launch does.  This is the form k_diag was compiled to.
static __device__ __forceinline__ amp_t cmul_diag(cplx d, amp_t a) {
    amp_t r;
    r.x = fma(a.x, d.re, -(a.y * d.im));
    r.y = fma(a.x, d.im, a.y * d.re);
    return r;
}

// acc + m * a, in two halves: the products with m.im first (inner), those with m.re on top (outer).  k_pass_tile issues
// the halves of its last column apart; everything else calls cfma.
static __device__ __forceinline__ amp_t cfma_inner(cplx m, amp_t a, amp_t acc) {
    amp_t r;
    r.x = fma(-m.im, a.y, acc.x);
    r.y = fma(m.im, a.x, acc.y);
    return r;
}
static __device__ __forceinline__ amp_t cfma_outer(cplx m, amp_t a, amp_t inner) {
    amp_t r;
    r.x = fma(m.re, a.x, inner.x);
    r.y = fma(m.re, a.y, inner.y);
    return r;
}
static __device__ __forceinline__ amp_t cfma(cplx m, amp_t a, amp_t acc) {
    return cfma_outer(m, a, cfma_inner(m, a, acc));
}

template <bool NT>
static __device__ __forceinline__ amp_t ld(const amp_t *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

template <bool NT>
static __device__ __forceinline__ void st(amp_t *p, amp_t v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

static __device__ __forceinline__ amp_t shfl_xor_amp(amp_t v, int lane_mask) {
    amp_t r;
    r.x = __shfl_xor(v.x, lane_mask, 64);
    r.y = __shfl_xor(v.y, lane_mask, 64);
    return r;
}

static __device__ __forceinline__ uint64_t insert_zero(uint64_t w, int p) {
    const uint64_t low = w & ((1ull << p) - 1ull);
    return ((w >> p) << (p + 1)) | low;
}

static __device__ __forceinline__ amp_t shfl_amp(amp_t v, int src_lane) {
    amp_t r;
    r.x = __shfl(v.x, src_lane, 64);
    r.y = __shfl(v.y, src_lane, 64);
    return r;
}

// The positions are 32-bit words on purpose.  The argument struct lives in the kernarg segment; a run-time index into
// a BYTE array there makes the compiler fetch the byte with a vector load (gfx950 has no sub-dword scalar loads)
// followed by s_waitcnt vmcnt(0) in front of every amplitude load -- which also drains every amplitude load already in
// flight (k_rdm ran at 1.3-2.3 TB/s that way; rocprof: 60-70 % of the wave cycles parked).  A dword array is indexed
// with s_load_dword.
template <class Args>
static __device__ __forceinline__ uint64_t deposit(uint64_t w, const Args &g) {
    for (int j = 0; j < g.nins; ++j) w = insert_zero(w, static_cast<int>(g.pos[j]));
    return w | g.or_mask;
}

// The LDS rows of k_dense_lds and k_seq_lds are private to a wave (a wave exchanges data with itself only), and the LDS
// executes one wave's instructions in order: no workgroup barrier is needed, only the compiler must keep the program order
// of the accesses (it does: they may alias) -- wave_sync() marks the spots.
static __device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

static __device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum of two doubles; result valid in thread 0.
static __device__ __forceinline__ void block_sum2(double &x, double &y) {
    __shared__ double sx[QSV_BLOCK / 64], sy[QSV_BLOCK / 64];
    x = wave_sum(x);
    y = wave_sum(y);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sx[wave] = x;
        sy[wave] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        x = 0.0;
        y = 0.0;
        for (int i = 0; i < QSV_BLOCK / 64; ++i) {
            x += sx[i];
            y += sy[i];
        }
    }
}

// ----------------------------------------------------------------------------------------------------
// host-side helpers
// ----------------------------------------------------------------------------------------------------
using qsv_layout::grid_for;   // workgroups of a grid-stride launch: with the launch rules it feeds, in qsv_layout.h

static int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qsv_fail(QSV_EHIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QSV_OK;
}

// The dispatches of one launch of g.W work items, at most `limit` each: launch(count) with g.w0 set to the range's start.
template <class Args, class Launch>
static int launch_ranges(Args &g, uint64_t limit, Launch &&launch) {
    for (const qsv_layout::Range &r : qsv_layout::dispatch_ranges(g.W, limit)) {
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

// Sum the first `blocks` pairs of partials on the host, in index order (deterministic).
static int sum_partials(qsv_state *st, int blocks, double *x, double *y) {
    QSV_HIP(hipMemcpyAsync(st->partials_host, st->partials, sizeof(double) * 2 * blocks, hipMemcpyDeviceToHost,
                           st->stream));
    QSV_HIP(hipStreamSynchronize(st->stream));
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < blocks; ++i) {
        sx += st->partials_host[2 * i];
        sy += st->partials_host[2 * i + 1];
    }
    *x = sx;
    if (y) *y = sy;
    return QSV_OK;
}

// A runtime bool or small int as a compile-time constant for a generic lambda: f(std::true_type / std::false_type), or
// f(std::integral_constant<int, v>) for v in LO..HI (any other value takes HI).  What f returns is passed on.
template <class F>
static auto with_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
template <int LO, int HI, class F>
static auto with_int(int v, F &&f) {
    if constexpr (LO < HI) {
        if (v != LO) return with_int<LO + 1, HI>(v, f);
    }
    return f(std::integral_constant<int, LO>{});
}
// The same for a power of two in LO..HI (items per thread, terms per pass, row tiles): only those are instantiated, and
// any other value takes HI (the callers' values come from ro_fit_items / ro_move_items, pauli_width and RdmPlan::T).
template <int LO, int HI, class F>
static auto with_pow2(int v, F &&f) {
    if constexpr (LO < HI) {
        if (v != LO) return with_pow2<LO * 2, HI>(v, f);
    }
    return f(std::integral_constant<int, LO>{});
}

// ---- streaming forms of the read-out / reshaping kernels and of k_diag_table_s ---------------------------------------
using qsv_readout_layout::RO_MIN_QUBITS;
static bool streaming_forms(const qsv_state *st) {   // QSV_OPT_READOUT_VARIANT = 1: the round-1 grid-stride forms
    return st->n >= RO_MIN_QUBITS && st->readout_variant != 1;
}
// amplitudes per thread of the kernels that move the register (collapse, insert, permute, table diagonals): one -- the
// plain copy kernel reaches 6.55 TB/s with one amplitude per thread and 6.05 with four (profiles/r03_copy_kernel.txt),
// and these kernels follow it (profiles/r03_readout_kernels.csv).  QSV_RO_ITEMS = 1 / 2 / 4 for measurements.
// items for a launch over `count` amplitudes: an AQL dispatch counts work-items in 32 bits (2^24 - 1 workgroups of 256),
// so registers beyond 2^32 amplitudes per launch take two or four per thread
static int ro_fit_items(int items, uint64_t count) {
    while (items < 4 && count / (static_cast<uint64_t>(QSV_BLOCK) * items) > 0x00ffffffull) items *= 2;
    return items;
}
static int ro_move_items() {
    static const int items = [] {
        const char *e = getenv("QSV_RO_ITEMS");
        const int v = e ? atoi(e) : 1;
        return v == 2 || v == 4 ? v : 1;   // (the table diagonals take two: 6.2 TB/s against 5.85 with one or four)
    }();
    return items;
}

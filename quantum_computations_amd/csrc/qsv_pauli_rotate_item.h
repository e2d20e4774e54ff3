// The item body of the Pauli-rotation passes: what one thread does to the pair {psi[i], psi[i ^ xmask]} (or to psi[i] alone
// in a diagonal pass) for the terms of a PauliRotateArgs.  Shared by k_pauli_rotate_group / k_pauli_adjoint_group
// (qsv_pauli.hip) and k_ens_pauli_rotate_group (qsv_sweep.hip), so that a member of an ensemble rounds exactly as a register
// of its own does.  Device functions only, static: each translation unit compiles its own copy.
#pragma once

#include "qsv_device.h"

// i^k v: a swap and signs of the real and imaginary part, never a multiplication (k is wave-uniform)
static __device__ __forceinline__ amp_t mul_i_pow(amp_t v, uint32_t k) {
    amp_t r;
    r.x = (k & 1u) ? v.y : v.x;
    r.y = (k & 1u) ? v.x : v.y;
    if (k == 1u || k == 2u) r.x = -r.x;
    if (k >= 2u) r.y = -r.y;
    return r;
}

// (c - i t) v
static __device__ __forceinline__ amp_t phase_amp(double c, double t, amp_t v) {
    amp_t r;
    r.x = fma(t, v.y, c * v.x);
    r.y = fma(-t, v.x, c * v.y);
    return r;
}

// Term t of the pass on one work item.  a = psi[i], b = psi[i ^ xmask] (unused when DIAG); s(j) = (-1)^{popcount(j & zmask)}
// and s(i ^ xmask) = s(i) s(xmask).  What a term is (diagonal or not, its power of i, whether its sign differs between the
// partners) is wave-uniform: scalar branches, no divergence.
template <bool DIAG>
static __device__ __forceinline__ void pauli_rotate_term(const qsv_readout_layout::PauliRotateArgs &g, int t, uint64_t i, amp_t &a, amp_t &b) {
    const uint64_t z = g.zmask[t];
    const double c = g.cs[t], sn = g.sn[t];
    const bool minus = __popcll(i & z) & 1;                   // s(i) = -1
    if (DIAG || ((g.diag >> t) & 1u)) {
        a = phase_amp(c, minus ? -sn : sn, a);
        if constexpr (!DIAG) {
            const bool differ = __popcll(g.xmask & z) & 1;
            b = phase_amp(c, (minus != differ) ? -sn : sn, b);
        }
    } else if constexpr (!DIAG) {
        const uint32_t n_y = (g.rot >> (2 * t)) & 3u, k = (n_y + 3u) & 3u;   // -i i^{nY} = i^k
        const bool differ = n_y & 1u;                                       // s(i') = (-1)^{nY} s(i)
        const double ta = (minus != differ) ? -sn : sn;   // sn s(i'), in front of b in a'
        const double tb = minus ? -sn : sn;               // sn s(i),  in front of a in b'
        const amp_t ra = mul_i_pow(a, k), rb = mul_i_pow(b, k);
        a = amp_t{fma(ta, rb.x, c * a.x), fma(ta, rb.y, c * a.y)};
        b = amp_t{fma(tb, ra.x, c * b.x), fma(tb, ra.y, c * b.y)};
    }
}

// The T terms of the pass on one work item, in the caller's order.
template <int T, bool DIAG>
static __device__ __forceinline__ void pauli_rotate_item(const qsv_readout_layout::PauliRotateArgs &g, uint64_t i, amp_t &a, amp_t &b) {
#pragma unroll
    for (int t = 0; t < T; ++t) pauli_rotate_term<DIAG>(g, t, i, a, b);
}

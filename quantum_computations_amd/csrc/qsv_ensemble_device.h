// What the translation units of the ensemble kernels share (qsv_ensemble.hip, qsv_sweep.hip, qsv_ensemble_adjoint.hip): who
// works on what in a unit of qsv_ensemble_layout.h, how a member's sums are formed, and what every ensemble call refuses.  Everything here is
// static; no __global__ function lives here.
#pragma once

#include "qsv_device.h"
#include "qsv_ensemble_layout.h"

// What a thread works on in unit `unit` (ens_thread of qsv_ensemble_layout.h, step for step).
struct Mine {
    uint64_t group, part, member, first, stride, items;
    uint32_t local;
    bool live;       // member < members
};
static __device__ __forceinline__ Mine mine(const qsv_ensemble_layout::EnsArgs &e, uint64_t unit) {
    Mine t;
    const uint32_t tid = threadIdx.x;
    const bool shared = e.item_bits < qsv_ensemble_layout::ENS_BLOCK_BITS;
    t.group = unit >> e.part_bits;
    t.part = unit & ((1ull << e.part_bits) - 1ull);
    t.member = (t.group << e.share_bits) + (shared ? tid >> e.item_bits : 0u);
    t.local = shared ? tid & ((1u << e.item_bits) - 1u) : tid;
    t.first = (t.part << qsv_ensemble_layout::ENS_BLOCK_BITS) + t.local;
    t.stride = static_cast<uint64_t>(QSV_BLOCK) << e.part_bits;
    t.items = 1ull << e.item_bits;
    t.live = t.member < e.members;
    return t;
}

// a 64-bit value that is the same in every lane of the wave, said so that the compiler can keep it in scalar registers
static __device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The sums of R doubles per thread, member by member: partials[(member * P + part) * R + e].  A member of fewer than 64 items
// is a run of aligned lanes and is summed by a butterfly over that run alone; from 64 items on the waves of a member are
// added in index order through LDS.  The order of every addition depends on the thread's place inside its member only.
// Every thread of the workgroup must call this (shuffles and barriers).
template <int R>
static __device__ __forceinline__ void member_store_sums(double (&v)[R], const qsv_ensemble_layout::EnsArgs &e, const Mine &t, double *__restrict__ partials) {
    const int segment = 1 << (e.item_bits < 6 ? e.item_bits : 6);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        if (o < segment) {     // wave-uniform
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] += __shfl_xor(v[r], o, 64);
        }
    }
    if (e.item_bits < 6) {     // one part; the first lane of the member's run holds its sums
        if (t.local == 0 && t.live) {
#pragma unroll
            for (int r = 0; r < R; ++r) partials[t.member * R + r] = v[r];
        }
        return;
    }
    __shared__ double sums[QSV_BLOCK / 64][R];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) sums[threadIdx.x >> 6][r] = v[r];
    }
    __syncthreads();
    const int wave_bits = e.item_bits - 6 < 2 ? e.item_bits - 6 : 2;     // log2 of the waves of one member in this workgroup
    const int sharing = (QSV_BLOCK / 64) >> wave_bits;                    // members in this workgroup
    if (threadIdx.x < sharing * R) {
        const int s = threadIdx.x / R, r = threadIdx.x % R;
        const uint64_t member = (t.group << e.share_bits) + s;
        if (member < e.members) {
            double sum = 0.0;
            for (int wv = 0; wv < (1 << wave_bits); ++wv) sum += sums[(s << wave_bits) + wv][r];
            partials[((member << e.part_bits) + t.part) * R + r] = sum;
        }
    }
    __syncthreads();     // the next unit writes sums again
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

// what every ensemble call refuses about the register and the member size
static int check_ensemble(const qsv_state *st, int member_qubits, int least) {
    if (!st) return qsv_fail(QSV_EINVAL, "null pointer");
    if (st->kind != 0) return qsv_fail(QSV_ESTATE, "this call needs a qubit register");
    if (!st->owns_data) return qsv_fail(QSV_EINVAL, "an ensemble lives in a register the library allocated, not in a view");
    if (member_qubits < least || member_qubits > st->n)
        return qsv_fail(QSV_EINVAL, "member_qubits must lie between " + std::to_string(least) + " and the register's " + std::to_string(st->n) + " qubits");
    return QSV_OK;
}

static int check_member_qubits(int member_qubits, int count, const int *qubits) {
    for (int i = 0; i < count; ++i) {
        if (qubits[i] < 0) return qsv_fail(QSV_EINVAL, "Non-negative index");
        if (qubits[i] >= member_qubits)
            return qsv_fail(QSV_EINVAL, "qubit index " + std::to_string(qubits[i]) + " out of range for members of " + std::to_string(member_qubits) + " qubits");
        for (int j = 0; j < i; ++j)
            if (qubits[i] == qubits[j]) return qsv_fail(QSV_EINVAL, "Indices must be distinct.");
    }
    return QSV_OK;
}

// A Pauli term list on member qubits, checked whole and turned into masks of member bits (qubit q is bit n - 1 - q).
static int parse_member_terms(int n, int n_terms, const int *term_offsets, const int *qubits, const char *paulis, std::vector<qsv_pauli_plan::Term> *terms) {
    terms->assign(static_cast<size_t>(n_terms), qsv_pauli_plan::Term{});
    for (int t = 0; t < n_terms; ++t) {
        const int first = term_offsets[t], len = term_offsets[t + 1] - first;
        if (first < 0 || len < 0) return qsv_fail(QSV_EINVAL, "Pauli term offsets must start at or above 0 and never decrease");
        if (len > 64) return qsv_fail(QSV_EINVAL, "bad Pauli string length");
        if (len > 0 && (!qubits || !paulis)) return qsv_fail(QSV_EINVAL, "null pointer");
        const int rc = check_member_qubits(n, len, len ? qubits + first : nullptr);
        if (rc) return rc;
        for (int j = first; j < first + len; ++j) {
            const uint64_t bit = 1ull << (n - 1 - qubits[j]);
            switch (paulis[j]) {
                case 'I': case 'i': break;
                case 'X': case 'x': (*terms)[t].xmask |= bit; break;
                case 'Z': case 'z': (*terms)[t].zmask |= bit; break;
                case 'Y': case 'y': (*terms)[t].xmask |= bit; (*terms)[t].zmask |= bit; break;
                default: return qsv_fail(QSV_EINVAL, "Pauli letters must be I, X, Y or Z");
            }
        }
    }
    return QSV_OK;
}

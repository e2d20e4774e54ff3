// Host-side planning of the diagonal-operator calls (qsv_diagonal.hip: qsv_diag_*, qsv_apply_diag_*, qsv_expect_diag,
// qsv_diag_transition, qsv_diag_phase_adjoint): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_diagonal_layout_host.py).
//
// A Z-only Pauli sum becomes a table of (mask, coefficient) rows in the caller's order; one write pass walks it for any
// number of terms.  The passes that reduce leave one partial per workgroup and slot in a scratch buffer, and the host
// combines a slot's partials in index order.  Everything here is index arithmetic.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qsv_diagonal_layout {

constexpr int DIAG_BLOCK = 256;             // = QSV_BLOCK
constexpr int DIAG_REDUCE_BLOCKS = 1024;    // = QSV_REDUCE_BLOCKS
constexpr uint64_t DIAG_MAX_BLOCKS = 0x00ffffffull;   // an AQL dispatch counts work-items in 32 bits (grid_for)
constexpr int DIAG_MAX_LETTERS = 64;

// ---- the term table -------------------------------------------------------------------------------------------------------
// One row per term, in the caller's order: d[i] += coeff * (-1)^popcount(i & zmask).  16 bytes, so a row is one scalar
// load of four dwords (the table is wave-uniform).
struct DiagTerm {
    uint64_t zmask;
    double coeff;
};
static_assert(sizeof(DiagTerm) == 16, "table row layout");

enum PackError { PACK_OK = 0, PACK_NULL, PACK_OFFSETS, PACK_LENGTH, PACK_RANGE, PACK_REPEAT, PACK_LETTER };

inline const char *pack_error_text(PackError e) {
    switch (e) {
        case PACK_OK: return "";
        case PACK_NULL: return "null pointer";
        case PACK_OFFSETS: return "term offsets must start at 0 and not decrease";
        case PACK_LENGTH: return "bad Pauli string length";
        case PACK_RANGE: return "qubit index out of range for the diagonal";
        case PACK_REPEAT: return "Indices must be distinct.";
        case PACK_LETTER: return "a diagonal operator takes the letters I and Z only";
    }
    return "?";
}

// Qubit q of n sits at bit n - 1 - q of the index, as in the register.  Term t is paulis[j] on qubits[j] for j in
// [term_offsets[t], term_offsets[t + 1]); coeffs may be NULL (all 1).  The whole list is checked before `out` is touched.
inline PackError pack_terms(int n_qubits, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                            const double *coeffs, std::vector<DiagTerm> *out) {
    if (n_terms < 0) return PACK_LENGTH;
    if (n_terms > 0 && !term_offsets) return PACK_NULL;
    if (n_terms > 0 && term_offsets[0] != 0) return PACK_OFFSETS;
    std::vector<DiagTerm> rows(static_cast<size_t>(n_terms));
    for (int t = 0; t < n_terms; ++t) {
        const int first = term_offsets[t], k = term_offsets[t + 1] - first;
        if (first < 0 || k < 0) return PACK_OFFSETS;
        if (k > DIAG_MAX_LETTERS) return PACK_LENGTH;
        if (k > 0 && (!qubits || !paulis)) return PACK_NULL;
        uint64_t seen = 0, zmask = 0;
        for (int j = first; j < first + k; ++j) {
            const int q = qubits[j];
            if (q < 0 || q >= n_qubits) return PACK_RANGE;
            const uint64_t bit = 1ull << (n_qubits - 1 - q);
            if (seen & bit) return PACK_REPEAT;
            seen |= bit;
            switch (paulis[j]) {
                case 'I': case 'i': break;
                case 'Z': case 'z': zmask |= bit; break;
                default: return PACK_LETTER;
            }
        }
        rows[t].zmask = zmask;
        rows[t].coeff = coeffs ? coeffs[t] : 1.0;
    }
    out->swap(rows);
    return PACK_OK;
}

// What the build kernel computes for index i, on the host: the same additions in the same order.
inline double table_value(const DiagTerm *rows, size_t n_rows, uint64_t i, double start) {
    double acc = start;
    for (size_t t = 0; t < n_rows; ++t) acc += (__builtin_popcountll(i & rows[t].zmask) & 1) ? -rows[t].coeff : rows[t].coeff;
    return acc;
}

// ---- grids ----------------------------------------------------------------------------------------------------------------
inline int blocks_for(uint64_t items, uint64_t cap) {
    uint64_t blocks = (items + DIAG_BLOCK - 1) / DIAG_BLOCK;
    blocks = std::max<uint64_t>(blocks, 1);
    if (cap > 0) blocks = std::min(blocks, cap);
    return static_cast<int>(std::min(blocks, DIAG_MAX_BLOCKS));
}
// A pass that reduces: at most DIAG_REDUCE_BLOCKS workgroups, fewer under QSV_OPT_GRID_CAP.  Loops from 2^18 items on.
inline int reduce_grid(uint64_t items, int grid_cap) {
    const uint64_t cap = grid_cap > 0 ? std::min<uint64_t>(grid_cap, DIAG_REDUCE_BLOCKS) : DIAG_REDUCE_BLOCKS;
    return blocks_for(items, cap);
}
// A pass that only streams: one item per thread unless QSV_OPT_GRID_CAP says otherwise.
inline int stream_grid(uint64_t items, int grid_cap) { return blocks_for(items, grid_cap > 0 ? static_cast<uint64_t>(grid_cap) : 0); }

// ---- scratch slices of the reducing kernels --------------------------------------------------------------------------------
// Every partial is 8 bytes (a double, or an index of k_diag_extrema); workgroup b writes slots [b * slots, (b + 1) * slots).
constexpr int EXPECT_SLOTS = 4;       // k_diag_expect: sum p, sum p d, sum p d^2, sum_{d <= threshold} p
constexpr int TRANSITION_SLOTS = 2;   // k_diag_transition, k_diag_phase_adjoint: re, im
constexpr int EXTREMA_SLOTS = 4;      // k_diag_extrema: min, argmin, max, argmax

struct ReducePlan {
    int grid = 0;
    int slots = 0;
    size_t words = 0;     // 8-byte words of scratch
    size_t bytes = 0;
};
inline ReducePlan reduce_plan(uint64_t items, int grid_cap, int slots) {
    ReducePlan p;
    p.grid = reduce_grid(items, grid_cap);
    p.slots = slots;
    p.words = static_cast<size_t>(p.grid) * slots;
    p.bytes = p.words * 8;
    return p;
}
inline size_t partial_index(const ReducePlan &p, int block, int slot) { return static_cast<size_t>(block) * p.slots + slot; }

// out[slot] = the sum over the workgroups, in index order.
inline void reduce_sums(const ReducePlan &p, const double *host, double *out) {
    for (int s = 0; s < p.slots; ++s) {
        double acc = 0.0;
        for (int b = 0; b < p.grid; ++b) acc += host[partial_index(p, b, s)];
        out[s] = acc;
    }
}

struct Extrema {
    double min = 0.0, max = 0.0;
    uint64_t argmin = 0, argmax = 0;
};
// Workgroup partials of k_diag_extrema combined in index order; ties go to the lowest index.
inline Extrema reduce_extrema(const ReducePlan &p, const uint64_t *host_words) {
    Extrema e;
    auto as_double = [](uint64_t w) {
        double v;
        __builtin_memcpy(&v, &w, 8);
        return v;
    };
    for (int b = 0; b < p.grid; ++b) {
        const double mn = as_double(host_words[partial_index(p, b, 0)]), mx = as_double(host_words[partial_index(p, b, 2)]);
        const uint64_t amn = host_words[partial_index(p, b, 1)], amx = host_words[partial_index(p, b, 3)];
        if (b == 0 || mn < e.min || (mn == e.min && amn < e.argmin)) {
            e.min = mn;
            e.argmin = amn;
        }
        if (b == 0 || mx > e.max || (mx == e.max && amx < e.argmax)) {
            e.max = mx;
            e.argmax = amx;
        }
    }
    return e;
}

}  // namespace qsv_diagonal_layout

// Pass planner of qsv_apply_pauli_rotations (qsv_api.hip): plain C++, no HIP, so that the host tests can compile it
// alone (tests/test_pauli_rotation_plan_host.py).
//
// A Pauli string acts on a basis state as  P|i> = i^{nY} (-1)^{popcount(i & zmask)} |i ^ xmask>  (qsv_pauli_plan.h), and
// P^2 = 1, so
//
//     exp(-i theta/2 P) = cos(theta/2) - i sin(theta/2) P
//
// only mixes the two amplitudes of each pair {i, i ^ xmask}; for xmask = 0 it is a diagonal phase.  With a = psi[i],
// b = psi[i'], i' = i ^ xmask, c = cos(theta/2), sn = sin(theta/2), s(j) = (-1)^{popcount(j & zmask)}:
//
//     term with the pair's xmask:   a' = c a - i sn i^{nY} s(i') b      b' = c b - i sn i^{nY} s(i) a
//     diagonal term (xmask = 0):    a' = (c - i sn s(i)) a              b' = (c - i sn s(i')) b
//
// Every rotation whose xmask is 0 or the pass's own xmask acts inside the same pairs: a thread that holds a pair applies
// a whole ordered run of such rotations in registers.  The planner below cuts the caller's list into such runs.  It is
// greedy and never reorders, so no commutation analysis is needed: the product is the caller's, factor by factor.
//
// The PIVOT of a pass is the HIGHEST set bit of its xmask (the expectation planner takes the lowest: it only reads).  A
// pass enumerates the i whose pivot bit is clear; with the highest flipped bit as pivot both i and i' run through
// contiguous ranges (i' = i + 2^pivot with the lower flipped bits permuting amplitudes inside the range), so loads and
// stores of a wave cover whole 128-byte lines whenever the pivot is at or above bit 3.
#pragma once

#include <stdint.h>

#include <vector>

#include "qsv_pauli_plan.h"

namespace qsv_pauli_rotation_plan {

using qsv_pauli_plan::Term;

// Rotations one launch of k_pauli_rotate_group applies.  Its widest instantiation is the cheapest per rotation
// ("Pauli rotations"), so the cap is not lowered.
constexpr int ROTATIONS_PER_PASS = 8;

struct Pass {
    uint64_t xmask = 0;                // the one non-zero xmask of the pass's terms; 0: every term is diagonal
    int pivot = -1;                    // highest set bit of xmask; -1 for a diagonal pass
    std::vector<int> index;            // position of each term in the caller's list, ascending and consecutive
    std::vector<uint64_t> term_xmask;  // per term: 0 or xmask
    std::vector<uint64_t> zmask;       // per term
    std::vector<int> n_y;              // popcount(term_xmask & zmask) per term
};

inline int highest_bit(uint64_t x) { return x ? 63 - __builtin_clzll(x) : -1; }

// Can `term` join a pass that flips `pass_xmask` and holds `count` terms?
inline bool joins(uint64_t pass_xmask, size_t count, const Term &term) {
    return count < static_cast<size_t>(ROTATIONS_PER_PASS) && (term.xmask == 0 || pass_xmask == 0 || term.xmask == pass_xmask);
}

inline std::vector<Pass> plan(const std::vector<Term> &terms) {
    std::vector<Pass> passes;
    for (size_t t = 0; t < terms.size(); ++t) {
        if (passes.empty() || !joins(passes.back().xmask, passes.back().index.size(), terms[t])) passes.emplace_back();
        Pass &p = passes.back();
        if (p.xmask == 0 && terms[t].xmask != 0) {   // a diagonal pass takes the xmask of the first term that flips
            p.xmask = terms[t].xmask;
            p.pivot = highest_bit(p.xmask);
        }
        p.index.push_back(static_cast<int>(t));
        p.term_xmask.push_back(terms[t].xmask);
        p.zmask.push_back(terms[t].zmask);
        p.n_y.push_back(qsv_pauli_plan::popcount64(terms[t].xmask & terms[t].zmask));
    }
    return passes;
}

}  // namespace qsv_pauli_rotation_plan

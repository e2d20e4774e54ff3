// Pass planner of qsv_expect_pauli_sum (qsv_api.hip): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_pauli_plan_host.py).
//
// A Pauli string acts on a basis state as  P|i> = i^{nY} (-1)^{popcount(i & zmask)} |i ^ xmask>  (Y = i X Z; xmask holds
// the X and Y positions, zmask the Z and Y positions, nY = popcount(xmask & zmask)).  Hence
//
//     <psi|P|psi> = i^{nY} sum_i s(i) c(i),      c(i) = conj(psi[i ^ xmask]) psi[i],   s(i) = (-1)^{popcount(i & zmask)}.
//
// 1. c(i) depends on xmask alone: every term with the same xmask needs the same products and differs in the signs only.
//    Such terms form a GROUP and share passes over the register (Z-only terms and the identity all have xmask = 0).
// 2. For xmask != 0 the indices i and i' = i ^ xmask are partners: c(i') = conj(c(i)) and s(i') = (-1)^{nY} s(i).  A pass
//    visits each pair once, through the i whose PIVOT bit (the lowest set bit of xmask) is clear, and the pair gives
//    s(i) (c + (-1)^{nY} conj(c)) = 2 s(i) Re c for even nY and 2 i s(i) Im c for odd nY.  Times i^{nY} that is real:
//        nY mod 4 = 0: +2 s Re c     1: -2 s Im c     2: -2 s Re c     3: +2 s Im c.
//    One real accumulator per term; pair_scale() below is the factor in front of it.
// 3. For xmask = 0 (the diagonal group) there are no partners: the pass walks every i with c(i) = |psi[i]|^2, nY = 0.
//
// A group is cut into passes of at most PAULI_TERMS_PER_PASS terms, which the kernel keeps in registers.
#pragma once

#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace qsv_pauli_plan {

// Terms one launch of k_expect_pauli_group accumulates.  Its widest instantiation (8 sign selections and 8 double
// accumulators per thread) holds the occupancy of the narrow ones ("Pauli sums"), so the cap is not lowered.
constexpr int PAULI_TERMS_PER_PASS = 8;

struct Term {
    uint64_t xmask = 0;   // register bits carrying X or Y
    uint64_t zmask = 0;   // register bits carrying Z or Y
};

struct Pass {
    uint64_t xmask = 0;
    int pivot = -1;                 // lowest set bit of xmask; -1: the diagonal group (xmask = 0)
    std::vector<uint64_t> zmask;    // per term of the pass, at most PAULI_TERMS_PER_PASS
    std::vector<int> n_y;           // popcount(xmask & zmask) per term
    std::vector<int> index;         // position of each term in the caller's list
};

inline int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// The factor in front of a term's accumulator (sum over visited i of s(i) Re c, or of s(i) Im c when n_y is odd).
inline double pair_scale(int pivot, int n_y) {
    if (pivot < 0) return 1.0;
    return ((n_y & 3) == 0 || (n_y & 3) == 3) ? 2.0 : -2.0;
}

// Groups in order of first appearance, the caller's order inside a group, each group cut into passes front to back.
inline std::vector<Pass> plan(const std::vector<Term> &terms) {
    std::vector<std::vector<int>> groups;
    std::unordered_map<uint64_t, size_t> group_of;
    for (size_t t = 0; t < terms.size(); ++t) {
        const auto found = group_of.find(terms[t].xmask);
        if (found == group_of.end()) {
            group_of.emplace(terms[t].xmask, groups.size());
            groups.push_back({static_cast<int>(t)});
        } else {
            groups[found->second].push_back(static_cast<int>(t));
        }
    }
    std::vector<Pass> passes;
    for (const std::vector<int> &members : groups) {
        const uint64_t xmask = terms[members[0]].xmask;
        for (size_t first = 0; first < members.size(); first += PAULI_TERMS_PER_PASS) {
            Pass p;
            p.xmask = xmask;
            p.pivot = xmask ? __builtin_ctzll(xmask) : -1;
            for (size_t m = first; m < members.size() && m < first + PAULI_TERMS_PER_PASS; ++m) {
                const uint64_t z = terms[members[m]].zmask;
                p.zmask.push_back(z);
                p.n_y.push_back(popcount64(xmask & z));
                p.index.push_back(members[m]);
            }
            passes.push_back(std::move(p));
        }
    }
    return passes;
}

}  // namespace qsv_pauli_plan

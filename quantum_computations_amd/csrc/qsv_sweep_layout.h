// Host-side launch shapes of the per-member parameter kernels (qsv_sweep.hip) and of the per-member adjoint walks
// (qsv_ensemble_adjoint.hip, at the end): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_sweep_layout_host.py, tests/test_ensemble_adjoint_layout_host.py).  DESIGN.md sections 27 and 30.
//
// The register is an ensemble (qsv_ensemble_layout.h): 2^b members of n qubits, member m at [m 2^n, (m + 1) 2^n).  A
// per-member rotation pass is a pass of qsv_pauli_rotation_plan.h planned on MEMBER-LOCAL masks and walked member by member:
// work item w of member m owns amplitude w of the member (diagonal pass, 2^n items) or the pair {i, i ^ xmask} with
// i = w with a zero inserted at the pivot (2^(n - 1) items).  The pivot is the highest flipped bit and lies below n, so i and
// i ^ xmask are both below 2^n: a partner never leaves its member.  The items are cut into the units of an UPDATE pass
// (apply_part_bits: one item per thread unless the grid cap says otherwise); how a member is cut depends on n and the grid
// cap alone, never on the number of members.
//
// The angles travel as one table of doubles, [members][n_terms][2] = cos(theta / 2), sin(theta / 2) of every term of the
// caller's list for every member.  A pass's terms are consecutive in that list (the planner never reorders), so the
// 2 x count doubles a member needs for a pass are contiguous: row m starts at m x 2 n_terms, the pass at 2 x first.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qsv_ensemble_layout.h"

namespace qsv_sweep_layout {

using qsv_ensemble_layout::EnsArgs;
using qsv_ensemble_layout::ENS_BLOCK_BITS;

// Passed by value (kernarg segment -> SGPRs): field order and sizes are ABI.
struct SweepArgs {
    uint64_t row_doubles;   // doubles of one member's row of the table: 2 n_terms
    uint32_t first;         // where the pass starts inside a row, in doubles: 2 x (index of its first term in the caller's list)
    int32_t count;          // terms of the pass, 1 .. 8; the slots beyond keep the padding (theta = 0) of pauli_rotate_args
};
static_assert(sizeof(SweepArgs) == 16, "kernel argument layout");

// The kernel fetches all T <= 8 slots of a pass without a branch and discards those beyond the pass's count: the table ends
// in padding so that the slots beyond the count of the last member's last pass lie inside the allocation.
constexpr int SWEEP_MAX_SLOTS = 8;                      // = qsv_pauli_rotation_plan::ROTATIONS_PER_PASS
constexpr size_t TABLE_PAD = 2 * SWEEP_MAX_SLOTS;
inline size_t table_doubles(uint64_t members, int n_terms) {
    return static_cast<size_t>(members) * 2 * static_cast<size_t>(n_terms) + (n_terms > 0 ? TABLE_PAD : 0);
}

inline SweepArgs sweep_args(int n_terms, int first_term, int count) {
    SweepArgs s;
    s.row_doubles = 2 * static_cast<uint64_t>(n_terms);
    s.first = 2 * static_cast<uint32_t>(first_term);
    s.count = count;
    return s;
}
// the double that holds cos (part 0) or sin (part 1) of slot t of the pass for `member`: what the kernel reads for every
// t < T (the pass's width, count <= T <= 8) and uses for t < count
inline size_t table_offset(const SweepArgs &s, uint64_t member, int t, int part) {
    return static_cast<size_t>(member) * s.row_doubles + s.first + 2 * static_cast<size_t>(t) + part;
}

// the units of a rotation pass: a diagonal pass has 2^n items per member, a flipping one 2^(n - 1)
inline int rotate_item_bits(int n, bool diag) { return diag ? n : n - 1; }
inline EnsArgs rotate_args(int n, uint64_t members, bool diag, int grid_cap) {
    const int item_bits = rotate_item_bits(n, diag);
    return qsv_ensemble_layout::ens_args(n, members, item_bits, qsv_ensemble_layout::apply_part_bits(item_bits, grid_cap));
}
// A wave (64 consecutive threads of a unit) lies in one member from 64 items per member on: the member index is then the
// same in all its lanes and the kernel may fetch the member's angles through the scalar path.  Below that the members share
// a wave and every lane fetches its own.
inline bool wave_in_one_member(const EnsArgs &e) { return e.item_bits >= 6; }
inline bool unit_in_one_member(const EnsArgs &e) { return e.item_bits >= ENS_BLOCK_BITS; }

// Non-temporal accesses as in the single-register pass (qsvk_pauli_rotate_passes): a pivot inside a 128-byte line (bits
// 0..2) leaves both halves of a line to one launch, which then uses cached accesses so that the halves meet in L2.
inline bool rotate_nontemporal(bool option, bool diag, int pivot) { return option && (diag || pivot >= 3); }

// the member-local amplitude pair of a work item (the kernel's own arithmetic)
inline uint64_t insert_zero(uint64_t w, int p) {
    const uint64_t low = w & ((1ull << p) - 1ull);
    return ((w >> p) << (p + 1)) | low;
}
// ... and back: the work item that owns a member-local index (for a flipping pass: of the pair's element with a clear pivot bit)
inline uint64_t item_of(uint64_t local, bool diag, int pivot) {
    if (diag) return local;
    const uint64_t low = local & ((1ull << pivot) - 1ull);
    return ((local >> (pivot + 1)) << pivot) | low;
}

// ---- read-out (k_ens_diag_expect): the units of a READ pass over 2^n items per member -----------------------------------------
constexpr int SWEEP_EXPECT_SLOTS = 4;     // sum p, sum p d, sum p d^2, sum_{d <= threshold} p
inline EnsArgs expect_args(int n, uint64_t members, int grid_cap) {
    return qsv_ensemble_layout::ens_args(n, members, n, qsv_ensemble_layout::part_bits(n, grid_cap));
}
// doubles of the scratch buffer: [members][4] results first, then [members][parts][4] partials
inline size_t expect_values(uint64_t members) { return static_cast<size_t>(members) * SWEEP_EXPECT_SLOTS; }
inline size_t expect_doubles(const EnsArgs &e) { return expect_values(e.members) + (static_cast<size_t>(e.members) << e.part_bits) * SWEEP_EXPECT_SLOTS; }

// ---- the per-member adjoint walk (qsv_ensemble_adjoint.hip) ---------------------------------------------
// k_ens_pauli_adjoint_group walks the items of a rotation pass (2^n per member in a diagonal pass, 2^(n - 1) otherwise) on
// the units of a READ pass: a thread takes 32 items where the member has them, so that the workgroup's sum of 2 T doubles
// (shuffles, LDS, two barriers) is paid once per 32 items and a member's parts never exceed the P_max(n) of the ensemble
// workspace, whose [members][P_max][16] partials hold the 2 x 8 doubles of the widest pass.  The cut of an update pass (one
// item per thread, items / 256 parts) would need 2^(n - 8) x 16 doubles per member and does not fit that workspace.  The cut
// depends on the items per member and the grid cap alone.
inline EnsArgs adjoint_args(int n, uint64_t members, bool diag, int grid_cap) {
    const int item_bits = rotate_item_bits(n, diag);
    return qsv_ensemble_layout::ens_args(n, members, item_bits, qsv_ensemble_layout::part_bits(item_bits, grid_cap));
}
// Threads of a member >= members (the last shared unit of a small ensemble) stay in the unit for the sums and contribute
// zeros; the row they fetch is the last member's, so that no fetch leaves the table.
inline uint64_t adjoint_fetch_member(const EnsArgs &e, uint64_t member) { return member < e.members ? member : e.members - 1; }
// The walk takes the terms of a pass in reverse order: slot t < count of the kernel is term count - 1 - t of the pass.  The
// slots beyond the count are fetched in place (inside the row or the padding) and discarded.
inline int adjoint_slot_term(const SweepArgs &s, int t) { return t < s.count ? s.count - 1 - t : t; }
inline size_t adjoint_table_offset(const SweepArgs &s, uint64_t member, int t, int part) {
    return table_offset(s, member, adjoint_slot_term(s, t), part);
}
// partials[((member << part_bits) + part) * 2 T + 2 t + {re, im}] (member_store_sums<2 T>), T = the pass's width
inline size_t adjoint_partial_offset(const EnsArgs &e, uint64_t member, uint64_t part, int width, int t, int c) {
    return ((static_cast<size_t>(member) << e.part_bits) + part) * 2 * width + 2 * static_cast<size_t>(t) + c;
}
inline size_t adjoint_partial_doubles(const EnsArgs &e, int width) { return (static_cast<size_t>(e.members) << e.part_bits) * 2 * width; }
inline bool adjoint_fits_workspace(const EnsArgs &e, int width) {
    const qsv_ensemble_layout::EnsWorkspace w = qsv_ensemble_layout::ens_workspace(e.n, e.members);
    return 2 * width <= qsv_ensemble_layout::ENS_ENTRIES && adjoint_partial_doubles(e, width) <= w.matrix - w.partials;
}
// What k_ens_adjoint_sum needs of a pass.  Passed by value: field order and sizes are ABI.
struct AdjointSumArgs {
    int32_t index[SWEEP_MAX_SLOTS];   // the caller's term behind slot t (-1: padding)
    int32_t width;                    // T of the pass
    int32_t parts;
    int32_t n_terms;
    int32_t pad;
};
static_assert(sizeof(AdjointSumArgs) == 48, "kernel argument layout");
// the scratch buffer of a walk, in doubles: the angle table, then the results [members][n_terms][2]
inline size_t adjoint_results_offset(uint64_t members, int n_terms) { return table_doubles(members, n_terms); }
inline size_t adjoint_results_doubles(uint64_t members, int n_terms) { return static_cast<size_t>(members) * static_cast<size_t>(n_terms) * 2; }
inline size_t adjoint_scratch_doubles(uint64_t members, int n_terms) {
    return adjoint_results_offset(members, n_terms) + adjoint_results_doubles(members, n_terms);
}

// ---- k_ens_inner, k_ens_diag_phase_adjoint: the units of a read pass over 2^n items per member, two sums per member ------------
constexpr int SWEEP_PAIR_SLOTS = 2;       // re, im
inline EnsArgs pair_args(int n, uint64_t members, int grid_cap) { return expect_args(n, members, grid_cap); }
inline size_t pair_partial_doubles(const EnsArgs &e) { return (static_cast<size_t>(e.members) << e.part_bits) * SWEEP_PAIR_SLOTS; }
// the sums [members][2] go to the first doubles of the workspace's [members][32] slots
inline size_t pair_values(uint64_t members) { return static_cast<size_t>(members) * SWEEP_PAIR_SLOTS; }

}  // namespace qsv_sweep_layout

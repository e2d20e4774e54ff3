// Host-side layout of the measurement and feed-forward calls of a trajectory ensemble (qsv_ensemble.hip:
// k_ens_measure_select, k_ens_apply_conditional): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_ensemble_control_layout_host.py).  DESIGN.md section 24.
//
// Every member of an ensemble owns one 64-bit word of CLASSICAL BITS, zero at creation.  A measurement writes its outcome
// to one bit of the word of its member; a conditional gate is taken by the members whose word satisfies
//     (word & all_of) == all_of && (word & none_of) == 0
// and by no other: the amplitudes of the others are neither read nor written.  The words live in a device allocation of
// their own, [members] uint64_t, beside the workspace of qsv_ensemble_layout.h and not inside it.
//
// k_ens_apply_conditional walks the units of an update pass (ens_args with apply_part_bits) exactly as
// k_ens_channel_apply does, and decides who takes the gate in one of two ways:
//   * a unit that lies in one member (item_bits >= 8): the member index is a function of the unit alone
//     (cond_unit_member), the word is loaded once per unit and the whole workgroup works on the unit or skips it;
//   * members that share a unit (item_bits < 8): every thread loads the word of its own member (ens_thread().member).
// The second way is safe for the lane form (kl > 0: amplitudes arrive by shfl_xor from other lanes of the wave) because of
// the rule of section 23: lanes are used only where n >= 6, and then a wave lies in one member, so every shfl_xor partner
// of a lane has the lane's own predicate and a wave is in the item loop as a whole or not at all.  With n < 6 there are
// no shuffles.  cond_partner_member states the rule; the layout test walks it.  The kernel has no barrier.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qsv_ensemble_layout.h"

namespace qsv_ensemble_control_layout {

using qsv_channel_layout::ChannelArgs;
using qsv_ensemble_layout::ENS_BLOCK_BITS;
using qsv_ensemble_layout::EnsArgs;
using qsv_ensemble_layout::ens_thread;

constexpr int ENS_CLASSICAL_BITS = 64;       // per member: one uint64_t

// ---- the classical bits ------------------------------------------------------------------------------------------------------
inline size_t bits_bytes(uint64_t members) { return sizeof(uint64_t) * static_cast<size_t>(members); }
inline bool takes(uint64_t word, uint64_t all_of, uint64_t none_of) { return (word & all_of) == all_of && (word & none_of) == 0; }
inline bool masks_ok(uint64_t all_of, uint64_t none_of) { return (all_of & none_of) == 0; }
// bit `bit` of `word` becomes `outcome`; bit < 0 leaves the word alone
inline uint64_t with_bit(uint64_t word, int bit, int outcome) {
    if (bit < 0) return word;
    const uint64_t mask = 1ull << bit;
    return outcome ? word | mask : word & ~mask;
}

// ---- kernel arguments, by value (kernarg segment): field order and sizes are ABI ---------------------------------------------
// The one matrix of a conditional gate, the same for every member: 4^k complex numbers, row-major, and the two masks.
struct ConditionalArgs {
    double m[32];
    uint64_t all_of, none_of;
    int32_t chunk_bits;    // cond_chunk_bits(units) where a unit lies in one member, else 0
    int32_t unused;
};
static_assert(sizeof(ConditionalArgs) == 280, "kernel argument layout");
// The two eigenvectors of a measurement, (Re, Im) of e_s[0] and e_s[1], what becomes of the qubit and where the outcome goes.
struct MeasureArgs {
    double eig[2][4];
    int32_t after;         // 0: the qubit is left in conj(e_s); 1: in |0>
    int32_t bit;           // 0 .. 63, -1 = the outcome is only logged
};
static_assert(sizeof(MeasureArgs) == 72, "kernel argument layout");

// ---- who decides what (the kernel spells out the same arithmetic) ----------------------------------------------------------------
// A unit lies in one member: one word per unit, the workgroup takes the unit or skips it as a whole.
inline bool cond_unit_uniform(const EnsArgs &e) { return e.item_bits >= ENS_BLOCK_BITS; }
// ... and that member, from the unit alone (share_bits is 0 there)
inline uint64_t cond_unit_member(const EnsArgs &e, uint64_t unit) { return (unit >> e.part_bits) << e.share_bits; }
// the member whose word thread `tid` of `unit` tests
inline uint64_t cond_thread_member(const EnsArgs &e, uint64_t unit, uint32_t tid) {
    return cond_unit_uniform(e) ? cond_unit_member(e, unit) : ens_thread(e, unit, tid).member;
}
// The member whose word the shfl_xor partner of a lane tests, for low combination `l` of the plan (l = 0: the lane itself).
// The rule: this is cond_thread_member of the lane, for every l the plan has.
inline uint64_t cond_partner_member(const EnsArgs &e, const ChannelArgs &g, uint64_t unit, uint32_t tid, int l) {
    const uint32_t partner = (tid & ~63u) | ((tid & 63u) ^ static_cast<uint32_t>(g.lxor[l]));
    return cond_thread_member(e, unit, partner);
}
// the lane form may be used with a per-thread predicate: a wave lies in one member
inline bool cond_lanes_safe(const EnsArgs &e, int kl) { return kl == 0 || e.item_bits >= 6; }

// ---- the grid, and how a workgroup walks its units --------------------------------------------------------------------------------
// Where a unit lies in one member a workgroup takes CHUNKS of 2^c consecutive units (c = cond_chunk_bits, at most 6): lane l
// of every wave loads the word of unit (chunk << c) + l, a ballot makes the predicates one wave-uniform mask and the wave
// works through the set bits.  A unit that is skipped costs its share of one load, not a workgroup launch and not a
// dependent load of its own.  Measured on 2^28 amplitudes against the dense gate on the same bits:
//   one workgroup per unit            nobody takes it 0.20 - 0.32 x, everybody 1.02 - 1.10 x  (profiles/r17_ensemble_control_one_workgroup_per_unit.json)
//   64 strided units per load         nobody 0.03 - 0.06 x, everybody 1.11 - 1.28 x           (profiles/r17_ensemble_control_strided_batches.json)
//   chunks of consecutive units       nobody 0.015 - 0.02 x, everybody 1.12 - 1.31 x          (profiles/r17_ensemble_control.json)
// A skip that costs a fifth of the gate is not a skip, so the chunks are what is built; what they cost the call that
// everybody takes is not understood (section 24 says what was looked at).  c is 0 up to 2^11 units -- a small register keeps
// one workgroup per unit and every CU busy -- and grows with the register so that at least 2^11 workgroups remain.
constexpr int COND_MAX_CHUNK_BITS = 6;       // the lanes of a wave
constexpr int COND_MIN_GRID_BITS = 11;     // 2048 workgroups of 256 threads: what 256 CUs hold at once
constexpr int cond_chunk_bits(uint64_t units) {
    int bits = 0;
    while (bits < COND_MAX_CHUNK_BITS && (units >> (bits + 1)) >= (1ull << COND_MIN_GRID_BITS)) ++bits;
    return bits;
}
inline uint64_t cond_chunks(const EnsArgs &e) {
    const int c = cond_unit_uniform(e) ? cond_chunk_bits(e.units) : 0;
    return (e.units + (1ull << c) - 1ull) >> c;
}
// workgroups: one per chunk (members that share a unit: one per unit), fewer under a grid cap; the kernel loops over the rest
inline int cond_grid(const EnsArgs &e, int grid_cap) {
    uint64_t blocks = std::min(cond_chunks(e), qsv_channel_layout::CH_MAX_BLOCKS);
    if (grid_cap > 0) blocks = std::min<uint64_t>(blocks, static_cast<uint64_t>(grid_cap));
    return static_cast<int>(std::max<uint64_t>(blocks, 1));
}
inline uint64_t cond_batch_unit(uint64_t chunk, uint32_t lane, int chunk_bits) { return (chunk << chunk_bits) + lane; }
// ... and the other way round: the workgroup, the chunk and the lane that look at a unit
struct CondVisit {
    uint64_t block, chunk;
    uint32_t lane;
};
inline CondVisit cond_visit_of(uint64_t unit, int chunk_bits, uint64_t grid) {
    CondVisit v;
    v.chunk = unit >> chunk_bits;
    v.lane = static_cast<uint32_t>(unit & ((1ull << chunk_bits) - 1ull));
    v.block = v.chunk % grid;
    return v;
}

}  // namespace qsv_ensemble_control_layout

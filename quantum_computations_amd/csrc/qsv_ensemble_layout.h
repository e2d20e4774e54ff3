// Host-side launch shapes of the trajectory-ensemble kernels (qsv_ensemble.hip): plain C++, no HIP, so that the host
// tests can compile it alone (tests/test_ensemble_layout_host.py).  DESIGN.md section 23.
//
// An ensemble is a register of 2^(n + b) amplitudes read as 2^b MEMBERS of n qubits: member m holds the amplitudes
// [m 2^n, (m + 1) 2^n).  Every kernel here walks work ITEMS of one member (for a channel: the member-local index with the
// high target bits removed, exactly the items of qsv_channel_layout.h on a register of 2^n amplitudes; for a Pauli pass:
// the member-local index, or the index with the pivot bit removed) and is launched over UNITS:
//
//   * a member of at least 256 items is cut into P PARTS and a unit is one part of one member: thread t of part p takes
//     the items p 256 + t, p 256 + t + P 256, ...  P is a power of two that depends on the items per member and on
//     QSV_OPT_GRID_CAP alone -- never on the number of members -- so what a member's sums are made of, and in which order,
//     is the same wherever the member sits and however many neighbours it has.  A read pass gives a thread 32 items
//     where the member has them (P = items / 8192, at most 128), so that the workgroup's sum of 4^k doubles is paid once
//     per 32 items: with P = items / 256 a two-qubit call on 4096 members of 16 qubits took 6.4 ms against a floor of
//     2.1, with this rule 2.3 (profiles/r16_ensemble_parts_per_256_items.json against profiles/r16_ensemble.json);
//   * members of fewer than 256 items have one part and SHARE a unit: 256 / items of them side by side, thread t working
//     on member (first of the unit) + t / items, item t % items.  Sums stop at the member: a member of fewer than 64 items
//     is summed by a butterfly over its own lanes, one of 64 or 128 items over its own waves.  No workgroup-level sum ever
//     mixes two members.
//
// The lane form (a target bit below 6 resolved with shfl_xor between the lanes of a wave) is used where n >= 6 and the
// register has not been switched to the round-1 forms: the items of a member are then a multiple of 64 (at most n - 6
// target bits can lie at or above bit 6), a wave is in the item loop as a whole and all its lanes belong to one member.
// (The single-register rule, n >= 14, is about streaming and is not copied.)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "qsv_channel_layout.h"

namespace qsv_ensemble_layout {

using qsv_channel_layout::CH_BLOCK;
using qsv_channel_layout::CH_LANE_BITS;
using qsv_channel_layout::CH_MAX_BLOCKS;
using qsv_channel_layout::ChannelPlan;

constexpr int ENS_BLOCK_BITS = 8;            // CH_BLOCK = 2^8 threads
constexpr int ENS_MAX_PART_BITS = 7;         // at most 128 parts per member
constexpr int ENS_READ_ITEM_BITS = 5;        // items per thread of a read pass before a member is cut into parts
constexpr int ENS_SELECT_LANES = 16;         // threads of k_ens_channel_select per member: 4^k, n_kraus <= 16
constexpr int ENS_LOG_SLOTS = 256;           // steps of the device log before it is drained
constexpr uint64_t ENS_LOG_BUDGET = 1ull << 22;   // member-steps the device log and the draw ring hold at most
static_assert(CH_BLOCK == 1 << ENS_BLOCK_BITS, "a workgroup is 256 threads");

// Passed by value (kernarg segment -> SGPRs): field order and sizes are ABI.
struct EnsArgs {
    uint64_t members;
    uint64_t units;        // member groups x parts
    int32_t n;             // qubits of a member
    int32_t item_bits;     // log2 of the items of one member
    int32_t part_bits;     // log2 P
    int32_t share_bits;    // log2 of the members that share a unit (0 unless items < 256)
};
static_assert(sizeof(EnsArgs) == 32, "kernel argument layout");

inline int floor_log2(uint64_t v) {
    int b = 0;
    while (v >>= 1) ++b;
    return b;
}

// log2 of the parts per member of a READ pass: items / (256 x 32), at most 128, at most the grid cap rounded down to a power of two
inline int part_bits(int item_bits, int grid_cap) {
    int bits = std::min(std::max(item_bits - ENS_BLOCK_BITS - ENS_READ_ITEM_BITS, 0), ENS_MAX_PART_BITS);
    if (grid_cap > 0) bits = std::min(bits, floor_log2(static_cast<uint64_t>(grid_cap)));
    return bits;
}
// ... and of an UPDATE pass: one item per thread unless the grid cap says otherwise
inline int apply_part_bits(int item_bits, int grid_cap) {
    int bits = std::max(item_bits - ENS_BLOCK_BITS, 0);
    if (grid_cap > 0) bits = std::min(bits, floor_log2(static_cast<uint64_t>(grid_cap)));
    return bits;
}

inline EnsArgs ens_args(int n, uint64_t members, int item_bits, int pbits) {
    EnsArgs e;
    e.members = members;
    e.n = n;
    e.item_bits = item_bits;
    e.part_bits = pbits;
    e.share_bits = std::max(ENS_BLOCK_BITS - item_bits, 0);
    const uint64_t groups = std::max<uint64_t>(members >> e.share_bits, 1);
    e.units = groups << pbits;
    return e;
}

// workgroups of a launch over e.units: the kernels loop over the units that are left
inline int ens_grid(const EnsArgs &e, int grid_cap) {
    uint64_t blocks = std::min(e.units, CH_MAX_BLOCKS);
    if (grid_cap > 0) blocks = std::min<uint64_t>(blocks, static_cast<uint64_t>(grid_cap));
    return static_cast<int>(std::max<uint64_t>(blocks, 1));
}

// ---- who works on what (the kernels spell out the same arithmetic) ---------------------------------------------------------
struct EnsThread {
    uint64_t member;       // may be >= members in the last unit of a small ensemble: such a thread does nothing
    uint64_t part;
    uint64_t first_item;   // then every stride-th
    uint64_t stride;
};
inline EnsThread ens_thread(const EnsArgs &e, uint64_t unit, uint32_t tid) {
    EnsThread t;
    const uint64_t group = unit >> e.part_bits;
    t.part = unit & ((1ull << e.part_bits) - 1ull);
    t.member = (group << e.share_bits) + (e.item_bits < ENS_BLOCK_BITS ? tid >> e.item_bits : 0u);
    const uint64_t local = e.item_bits < ENS_BLOCK_BITS ? tid & ((1u << e.item_bits) - 1u) : tid;
    t.first_item = (t.part << ENS_BLOCK_BITS) + local;
    t.stride = static_cast<uint64_t>(CH_BLOCK) << e.part_bits;
    return t;
}
// ... and the other way round: which member, part, unit and thread own a work item of a member
struct EnsOwner {
    uint64_t part, unit;
    uint32_t tid;
};
inline EnsOwner ens_owner(const EnsArgs &e, uint64_t member, uint64_t item) {
    EnsOwner o;
    o.part = (item >> ENS_BLOCK_BITS) & ((1ull << e.part_bits) - 1ull);
    o.unit = ((member >> e.share_bits) << e.part_bits) | o.part;
    o.tid = e.item_bits < ENS_BLOCK_BITS ? static_cast<uint32_t>(((member & ((1ull << e.share_bits) - 1ull)) << e.item_bits) | item)
                                         : static_cast<uint32_t>(item & (CH_BLOCK - 1));
    return o;
}
// the member and the member-local index of an amplitude of the register
inline uint64_t ens_member_of(int n, uint64_t amplitude) { return amplitude >> n; }
inline uint64_t ens_local_of(int n, uint64_t amplitude) { return amplitude & ((1ull << n) - 1ull); }
// the work item that holds a member-local index: the index with the high target bits taken out (inverse of item_base)
inline uint64_t ens_item_of(const qsv_channel_layout::ChannelArgs &g, uint64_t local) {
    for (int j = g.nins - 1; j >= 0; --j) {
        const uint64_t low = local & ((1ull << g.pos[j]) - 1ull);
        local = ((local >> (g.pos[j] + 1)) << g.pos[j]) | low;
    }
    return local;
}

// lanes of a wave that are summed together (a butterfly over aligned runs of this many lanes), and the waves per member
inline int ens_segment_lanes(const EnsArgs &e) { return 1 << std::min(e.item_bits, 6); }
inline int ens_waves_per_member(const EnsArgs &e) { return e.item_bits <= 6 ? 1 : std::min(1 << (e.item_bits - 6), CH_BLOCK / 64); }

// ---- channels ----------------------------------------------------------------------------------------------------------------
inline bool ens_lanes(int n, bool streaming_allowed) { return streaming_allowed && n >= CH_LANE_BITS; }

// The member-local plan: channel_plan's index arithmetic on a register of 2^n amplitudes, with the ensemble's lane rule.
inline ChannelPlan ens_channel_plan(int n, int k, const int *bits, bool lanes) {
    // channel_plan takes lanes where streaming && n >= 14: lend it a qubit count that passes, the arithmetic uses bits only
    return qsv_channel_layout::channel_plan(lanes ? std::max(n, qsv_channel_layout::CH_MIN_STREAM_QUBITS) : 0, 1ull << n, k, bits, lanes);
}

// P(n, k, grid cap) of the read pass for the worst and best placement of the target bits is part_bits(n - kh, cap).
inline int channel_part_bits(int n, int kh, int grid_cap) { return part_bits(n - kh, grid_cap); }

// ---- the workspace of a register's ensemble calls (one device allocation, in doubles) -----------------------------------------
constexpr int ENS_ENTRIES = 16;              // room per part: 4^k reals, k <= 2; 8 Pauli terms
struct EnsWorkspace {
    uint64_t members = 0;
    int slots = 0;            // steps the log holds: ENS_LOG_SLOTS, fewer for very many members (at least 1)
    size_t partials = 0;      // [members][P_max(n)][16]
    size_t matrix = 0;        // [members][32]
    size_t draws = 0;         // [members][2]: u, forced branch (-1 = draw)
    size_t log = 0;           // [slots][members][2]: branch, probability
    size_t doubles = 0;
};
inline EnsWorkspace ens_workspace(int n, uint64_t members) {
    EnsWorkspace w;
    w.members = members;
    w.slots = static_cast<int>(std::min<uint64_t>(ENS_LOG_SLOTS, std::max<uint64_t>(ENS_LOG_BUDGET / members, 1)));
    const size_t parts = size_t(1) << part_bits(n, 0);     // the most any pass over a member of n qubits is cut into
    w.partials = 0;
    w.matrix = w.partials + static_cast<size_t>(members) * parts * ENS_ENTRIES;
    w.draws = w.matrix + static_cast<size_t>(members) * 32;
    w.log = w.draws + static_cast<size_t>(members) * 2;
    w.doubles = w.log + static_cast<size_t>(w.slots) * members * 2;
    return w;
}

}  // namespace qsv_ensemble_layout

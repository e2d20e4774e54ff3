// Pass planner of the deferred gate queue (qsv_api.hip): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_defer_plan_host.py).
//
// A register of 2^n amplitudes is cut into tiles of 2^12: the tile always holds bits 0..5 (every tile row is 64 consecutive
// amplitudes, one 1 KiB run in HBM) and six further bits.  A PASS brings every tile into LDS once, applies an ordered list of
// queued gates to it and writes it back (k_pass_tile): one round trip over HBM instead of one per gate.  A gate fits a pass
// when its target bits are tile bits; its control bits may lie anywhere -- inside the tile they select amplitudes, outside it
// they select whole tiles (the same bits for every amplitude of a tile).  A CZ on two bits is all controls, a CX's control
// may stay outside the tile.  Inside the kernel the gates of a pass are applied in GROUPS (cut_groups): consecutive gates whose
// targets fit four tile bits are applied in registers, 16 amplitudes per thread, with one LDS round trip per group.
//
// Ordering.  The gates of a pass keep queue order, with one exception: a gate that is a signed permutation (CX, CZ, SWAP,
// X, Z: every matrix entry 0 or +-1) may move ahead of earlier queued gates that act on none of its qubits.  Such a gate
// computes nothing that rounds, so applying it earlier changes no bit of the result.  Nothing else is reordered and no two
// gates are multiplied together: every gate is applied with the arithmetic of its own per-gate kernel.
#pragma once

#include <stdint.h>

#include <vector>

namespace qsv_plan {

constexpr int TILE_BITS = 12;                       // amplitudes per tile: 2^12 = 64 KiB of complex128
constexpr int LANE_BITS = 6;                        // bits 0..5 are always tile bits
constexpr int HIGH_BITS = TILE_BITS - LANE_BITS;    // further tile bits chosen per pass
constexpr int MAX_PASS_GATES = 64;                  // gates per pass (the kernel keeps one activity bit per gate)
constexpr uint64_t LOW_MASK = (1ull << LANE_BITS) - 1;

constexpr int REG_BITS = 4;                         // tile bits a thread of k_pass_tile holds in registers (16 amplitudes)

// Cost model, in units of one full pass of a per-gate kernel over the register (k_dense_tile12<1> at n = 28: 1.31 ms).
// k_pass_tile applies a pass's gates in GROUPS (cut_groups below): one LDS round trip and one barrier per group, the
// gates of a group in registers.  On the benchmark circuit (profiles/r05_pass_costs.txt): 1.77-3.67 ms for 6-20 gates in
// 2-5 groups, least squares 0.85 ms + 0.160 ms per group + 0.101 ms per gate (0.65 + 0.122 per group + 0.077 per gate in
// these units); the intercept is rounded up to one full pass, below which no pass over HBM can go.  A pass costs
// PASS_BASE times the fraction of tiles it loads plus PASS_PER_GROUP per group plus PASS_PER_GATE per gate; a gate
// launched on its own costs what qsv_api.hip (plan_gate) gives its kind.
constexpr float PASS_BASE = 1.0f;
constexpr float PASS_PER_GROUP = 0.12f;
constexpr float PASS_PER_GATE = 0.08f;

struct Gate {
    uint64_t need = 0;   // register bits that must be tile bits (target legs)
    uint64_t ctrl = 0;   // register bits that must be 1 for the gate to act (controls, the bits of a phase)
    bool exact = false;  // a signed permutation: may move ahead of earlier gates on disjoint bits
    float cost = 1.0f;   // its per-gate launch, in full passes
    bool dense = true;   // false: a diagonal gate (it scales amplitudes in place and needs no register bits of a group)
};

struct Pass {
    uint64_t tile = 0;          // the pass's tile bits >= 6 (min(6, n - 6) of them)
    std::vector<int> gates;     // queue indices, in application order
    bool fused = false;         // true: one k_pass_tile launch; false: gates[0] (always queue index 0) on its own kernel
};

inline int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// Tile index (0..11) of register bit b in a pass whose tile bits are 0..5 and `tile`; -1: b is not a tile bit.
inline int tile_index(int b, uint64_t tile) {
    if (b < LANE_BITS) return b;
    if (b >= 64 || !((tile >> b) & 1)) return -1;
    return LANE_BITS + popcount64(tile & ((1ull << b) - 1));
}

// A gate's control bits in a pass: those inside the tile as tile indices (they select amplitudes), the others as
// register bits (they select whole tiles: the gate acts on a tile iff all of them are 1 in its base index).
struct ControlMasks {
    uint32_t inside = 0;
    uint64_t outside = 0;
};
inline ControlMasks control_masks(uint64_t ctrl, uint64_t tile) {
    ControlMasks cm;
    for (int b = 0; b < 64; ++b) {
        if (!((ctrl >> b) & 1)) continue;
        const int t = tile_index(b, tile);
        if (t >= 0) cm.inside |= 1u << t;
        else cm.outside |= 1ull << b;
    }
    return cm;
}

// Fraction of the tiles on which at least one gate of the pass acts (an upper bound: overlaps are not subtracted).
inline float active_fraction(const std::vector<Gate> &q, const std::vector<int> &gates, uint64_t tile) {
    float frac = 0.0f;
    for (int i : gates) {
        const int outside = popcount64(q[i].ctrl & ~tile & ~LOW_MASK);
        frac += 1.0f / static_cast<float>(1ull << (outside < 60 ? outside : 60));
        if (frac >= 1.0f) return 1.0f;
    }
    return frac;
}

// One group of a pass: gates [first, first + count) of the pass's ordered list, applied on the 16 amplitudes of the four
// tile indices reg[] (ascending) that a thread holds in registers.
struct Group {
    int first = 0, count = 0;
    int reg[REG_BITS] = {0, 0, 0, 0};
};

// Cut the gates of one pass into groups.  need[i]: the target bits of gate i as a mask of tile indices (0 .. tile_bits -
// 1), in application order; a gate without targets (phases, CZ, diagonal gates: they only scale amplitudes, wherever
// their bits sit) has need 0.  A group is a maximal run of consecutive gates whose targets together occupy at most REG_BITS
// tile indices: a gate joins the open group when it fits, otherwise it closes the group and opens the next.  Nothing is
// reordered.  A gate without targets always fits, so it never opens a group unless it is first in the pass.  A group's
// register bits are completed to REG_BITS with the highest unused tile indices: the low tile bits then stay thread bits,
// so that consecutive lanes read consecutive 16-byte amplitudes of LDS.
inline std::vector<Group> cut_groups(const std::vector<uint32_t> &need, int tile_bits = TILE_BITS) {
    std::vector<Group> out;
    std::vector<uint32_t> masks;
    uint32_t cur = 0;
    for (int i = 0; i < static_cast<int>(need.size()); ++i) {
        const uint32_t grown = cur | need[i];
        if (out.empty() || popcount64(grown) > REG_BITS) {
            if (!out.empty()) masks.push_back(cur);
            Group g;
            g.first = i;
            out.push_back(g);
            cur = need[i];
        } else {
            cur = grown;
        }
        ++out.back().count;
    }
    if (!out.empty()) masks.push_back(cur);
    for (size_t k = 0; k < out.size(); ++k) {
        uint32_t m = masks[k];
        for (int t = tile_bits - 1; t >= 0 && popcount64(m) < REG_BITS; --t)
            if (!((m >> t) & 1)) m |= 1u << t;
        int w = 0;
        for (int t = 0; t < tile_bits && w < REG_BITS; ++t)
            if ((m >> t) & 1) out[k].reg[w++] = t;
    }
    return out;
}

// A gate's targets as tile indices for cut_groups: `need` restricted to dense gates (has_targets), 0 for the others.
inline uint32_t need_in_tile(uint64_t need, uint64_t tile) {
    uint32_t m = 0;
    for (int b = 0; b < 64; ++b)
        if ((need >> b) & 1) {
            const int t = tile_index(b, tile);
            if (t >= 0) m |= 1u << t;
        }
    return m;
}

inline int count_groups(const std::vector<Gate> &q, const std::vector<int> &gates, uint64_t tile) {
    std::vector<uint32_t> need;
    need.reserve(gates.size());
    for (int i : gates) need.push_back(q[i].dense ? need_in_tile(q[i].need, tile) : 0u);
    return static_cast<int>(cut_groups(need).size());
}

inline float pass_cost(const std::vector<Gate> &q, const std::vector<int> &gates, uint64_t tile) {
    return PASS_BASE * active_fraction(q, gates, tile) + PASS_PER_GROUP * static_cast<float>(count_groups(q, gates, tile)) +
           PASS_PER_GATE * static_cast<float>(gates.size());
}

// The first pass of the queue q on an n-qubit register (n >= TILE_BITS): gate 0 and every later gate that can join it in
// the order rules above while the targets of all of them fit six tile bits.  Greedy, first come first served.
inline Pass plan_first(const std::vector<Gate> &q, int n) {
    Pass p;
    if (q.empty()) return p;
    const uint64_t all = n >= 64 ? ~0ull : (1ull << n) - 1;
    const int high_bits = n - LANE_BITS < HIGH_BITS ? n - LANE_BITS : HIGH_BITS;
    uint64_t tile = 0, blocked = 0;
    bool left_behind = false;
    for (int i = 0; i < static_cast<int>(q.size()) && static_cast<int>(p.gates.size()) < MAX_PASS_GATES; ++i) {
        const Gate &g = q[i];
        const uint64_t bits = g.need | g.ctrl;
        const bool order_ok = !left_behind || (g.exact && (bits & blocked) == 0);
        const uint64_t grown = tile | (g.need & ~LOW_MASK);
        if (order_ok && popcount64(grown) <= high_bits) {
            tile = grown;
            p.gates.push_back(i);
        } else {
            left_behind = true;
            blocked |= bits;
        }
    }
    // complete the tile with the lowest unused bits: a control that becomes a tile bit selects amplitudes, not tiles
    for (int b = LANE_BITS; b < n && popcount64(tile) < high_bits; ++b)
        if (!((tile >> b) & 1)) tile |= 1ull << b;
    p.tile = tile & all;
    float alone = 0.0f;
    for (int i : p.gates) alone += q[i].cost;
    p.fused = p.gates.size() >= 2 && pass_cost(q, p.gates, p.tile) < alone;
    if (!p.fused) p.gates.resize(1);
    return p;
}

// What the library launches for gates queued one by one: once `window` gates are pending the first pass is launched (the
// GPU works while the host queues), and a flush at the end launches the rest.  Indices refer to q.
inline std::vector<Pass> plan_stream(const std::vector<Gate> &q, int n, size_t window) {
    std::vector<Pass> out;
    std::vector<Gate> pending;
    std::vector<int> idx;
    auto launch_first = [&]() {
        Pass p = plan_first(pending, n);
        std::vector<bool> taken(pending.size(), false);
        for (int &i : p.gates) {
            taken[i] = true;
            i = idx[i];
        }
        size_t w = 0;
        for (size_t i = 0; i < pending.size(); ++i)
            if (!taken[i]) {
                pending[w] = pending[i];
                idx[w++] = idx[i];
            }
        pending.resize(w);
        idx.resize(w);
        out.push_back(std::move(p));
    };
    for (size_t i = 0; i < q.size(); ++i) {
        pending.push_back(q[i]);
        idx.push_back(static_cast<int>(i));
        if (pending.size() >= window) launch_first();
    }
    while (!pending.empty()) launch_first();
    return out;
}

}  // namespace qsv_plan

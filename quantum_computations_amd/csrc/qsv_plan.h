// Pass planner of the deferred gate queue (qsv_api.hip): plain C++, no HIP, so that the host tests can compile it alone
// (tests/test_defer_plan_host.py).
//
// A register of 2^n amplitudes is cut into tiles of 2^12: the tile always holds bits 0..5 (every tile row is 64 consecutive
// amplitudes, one 1 KiB run in HBM) and six further bits.  A PASS brings every tile into LDS once, applies an ordered list of
// queued gates to it and writes it back (k_pass_tile): one round trip over HBM instead of one per gate.  A gate fits a pass
// when its target bits are tile bits; its control bits may lie anywhere -- inside the tile they select amplitudes, outside it
// they select whole tiles (the same bits for every amplitude of a tile).  A CZ on two bits is all controls, a CX's control
// may stay outside the tile.
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

// Cost model, in units of one full pass of a per-gate kernel over the register (k_dense_tile12<1> at n = 28: 1.31 ms).
// k_pass_tile on the benchmark circuit (profiles/r04_pass_costs.txt): 1.95-4.48 ms for 6-20 gates, least squares
// 0.99 ms + 0.172 ms per gate (0.75 + 0.131 per gate in these units); the intercept is rounded up to one full pass, below
// which no pass over HBM can go.  A pass costs PASS_BASE times the fraction of tiles it loads plus PASS_PER_GATE per
// gate; a gate launched on its own costs what qsv_api.hip (plan_gate) gives its kind.
constexpr float PASS_BASE = 1.0f;
constexpr float PASS_PER_GATE = 0.13f;

struct Gate {
    uint64_t need = 0;   // register bits that must be tile bits (target legs)
    uint64_t ctrl = 0;   // register bits that must be 1 for the gate to act (controls, the bits of a phase)
    bool exact = false;  // a signed permutation: may move ahead of earlier gates on disjoint bits
    float cost = 1.0f;   // its per-gate launch, in full passes
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

inline float pass_cost(const std::vector<Gate> &q, const std::vector<int> &gates, uint64_t tile) {
    return PASS_BASE * active_fraction(q, gates, tile) + PASS_PER_GATE * static_cast<float>(gates.size());
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

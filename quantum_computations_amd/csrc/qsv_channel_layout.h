// Host-side launch shapes of the Kraus-channel kernels (qsv_channel.hip: k_channel_rdm, k_channel_select,
// k_channel_apply): plain C++, no HIP, so that the host tests can compile it alone (tests/test_channel_layout_host.py).
//
// A channel acts on k = 1 or 2 target bits.  On a streaming register (>= 2^14 amplitudes) a target bit below 6 is a LANE
// bit: the 2^kl amplitudes it spans sit in other lanes of the same wave and arrive by shfl_xor.  A target bit from 6 up
// -- and every target bit of a small register -- is a HIGH bit: a thread loads the 2^kh amplitudes it spans itself.  A
// work item is the index with the kh high bits removed, so consecutive items are consecutive amplitudes and every wave
// access is one whole 1 KiB segment.  Everything here is index arithmetic.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

namespace qsv_channel_layout {

constexpr int CH_BLOCK = 256;               // = QSV_BLOCK
constexpr int CH_REDUCE_BLOCKS = 1024;      // = QSV_REDUCE_BLOCKS
constexpr int CH_LANE_BITS = 6;             // = QSV_LANE_BITS
constexpr int CH_MIN_STREAM_QUBITS = 14;    // = RO_MIN_QUBITS: below this every target bit is a high bit
constexpr uint64_t CH_MAX_BLOCKS = 0x00ffffffull;   // an AQL dispatch counts work-items in 32 bits (grid_for)
constexpr int CH_MAX_KRAUS = 16;
constexpr int CH_LOG_SLOTS = 256;           // device slots of a register's branch log before it is drained to the host

// Passed by value (kernarg segment -> SGPRs): field order and sizes are ABI.
struct ChannelArgs {
    uint64_t W;          // work items = amps >> kh
    uint64_t or_mask;    // unused (0); lets deposit() serve this struct too
    uint64_t hoff[4];   // offset of high combination h (bit i of h <-> pos[i])
    int32_t nins;        // kh
    int32_t kl;
    uint32_t pos[2];     // the high target bits, ascending: a zero is inserted there
    int32_t lxor[4];     // lane xor mask of low combination l (bit i of l <-> lbit[i])
    int32_t lbit[2];     // the low target bits, ascending
    int32_t ghi[4];      // what high combination h adds to the group index (the row / column of the 2^k x 2^k matrix)
    int32_t glo[4];      // what low combination l adds to it
};
static_assert(sizeof(ChannelArgs) == 16 + 32 + 8 + 8 + 16 + 8 + 16 + 16, "kernel argument layout");

struct ChannelPlan {
    int k = 0, kh = 0, kl = 0, D = 0;
    ChannelArgs g;
};

// bits[j] = index bit of leg j; leg 0 is the most significant bit of the matrix index, as everywhere in qsv.h.
inline ChannelPlan channel_plan(int n, uint64_t amps, int k, const int *bits, bool streaming) {
    ChannelPlan p;
    p.k = k;
    p.D = 1 << k;
    ChannelArgs &g = p.g;
    memset(&g, 0, sizeof(g));
    const bool lanes = streaming && n >= CH_MIN_STREAM_QUBITS;
    int order[2] = {0, 1};
    if (k == 2 && bits[1] < bits[0]) std::swap(order[0], order[1]);      // legs by ascending bit
    int hweight[2] = {0, 0}, lweight[2] = {0, 0};
    for (int i = 0; i < k; ++i) {
        const int leg = order[i], bit = bits[leg], weight = 1 << (k - 1 - leg);
        if (lanes && bit < CH_LANE_BITS) {
            g.lbit[p.kl] = bit;
            lweight[p.kl++] = weight;
        } else {
            g.pos[p.kh] = static_cast<uint32_t>(bit);
            hweight[p.kh++] = weight;
        }
    }
    g.nins = p.kh;
    g.kl = p.kl;
    g.W = amps >> p.kh;
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 2; ++i)
            if ((c >> i) & 1) {
                if (i < p.kh) {
                    g.hoff[c] |= 1ull << g.pos[i];
                    g.ghi[c] |= hweight[i];
                }
                if (i < p.kl) {
                    g.lxor[c] |= 1 << g.lbit[i];
                    g.glo[c] |= lweight[i];
                }
            }
    return p;
}

// the amplitude index of work item w with every high bit 0 (the kernels' deposit())
inline uint64_t item_base(const ChannelArgs &g, uint64_t w) {
    for (int j = 0; j < g.nins; ++j) {
        const uint64_t low = w & ((1ull << g.pos[j]) - 1ull);
        w = ((w >> g.pos[j]) << (g.pos[j] + 1)) | low;
    }
    return w;
}
// the low combination a lane owns
inline int lane_combination(const ChannelArgs &g, uint32_t lane) {
    int l = 0;
    for (int i = 0; i < g.kl; ++i) l |= static_cast<int>((lane >> g.lbit[i]) & 1u) << i;
    return l;
}

// ---- grids ----------------------------------------------------------------------------------------------------------------
inline int blocks_for(uint64_t items, uint64_t cap) {
    uint64_t blocks = (items + CH_BLOCK - 1) / CH_BLOCK;
    blocks = std::max<uint64_t>(blocks, 1);
    if (cap > 0) blocks = std::min(blocks, cap);
    return static_cast<int>(std::min(blocks, CH_MAX_BLOCKS));
}
// the read pass: at most CH_REDUCE_BLOCKS workgroups, fewer under QSV_OPT_GRID_CAP; loops over the rest
inline int rdm_grid(uint64_t items, int grid_cap) {
    return blocks_for(items, grid_cap > 0 ? std::min<uint64_t>(grid_cap, CH_REDUCE_BLOCKS) : CH_REDUCE_BLOCKS);
}
// the update pass: one item per thread unless QSV_OPT_GRID_CAP says otherwise
inline int apply_grid(uint64_t items, int grid_cap) { return blocks_for(items, grid_cap > 0 ? static_cast<uint64_t>(grid_cap) : 0); }

// ---- the reduced density matrix as real numbers -----------------------------------------------------------------------------
// D diagonal entries, then (Re, Im) of rho[r][c] = sum a_r conj(a_c) for r < c in row-major order: 4 numbers for k = 1,
// 16 for k = 2.
inline int rdm_entries(int D) { return D * D; }
inline int rdm_pair_slot(int D, int r, int c) {   // r < c
    int before = 0;
    for (int a = 0; a < r; ++a) before += D - 1 - a;
    return D + 2 * (before + (c - r - 1));
}

// ---- the workspace of a register's channel calls (one device allocation, in doubles) -----------------------------------------
constexpr size_t WS_PARTIALS = 0;                                        // [CH_REDUCE_BLOCKS][16]
constexpr size_t WS_RHO = WS_PARTIALS + size_t(CH_REDUCE_BLOCKS) * 16;   // [16]
constexpr size_t WS_MATRIX = WS_RHO + 16;                                // the chosen K_j, scaled: [32]
constexpr size_t WS_LOG = WS_MATRIX + 32;                                // [CH_LOG_SLOTS][2]: branch, probability
constexpr size_t WS_DOUBLES = WS_LOG + size_t(CH_LOG_SLOTS) * 2;

// ---- the branch rule, on the host (mixed-unitary channels; the select kernel spells out the same steps) ---------------------
// The first j with w_0 + ... + w_j > u * total, else the last j with w_j > 0, else 0.
inline int pick_branch(const double *w, int count, double u, double *total_out) {
    double total = 0.0;
    for (int j = 0; j < count; ++j) total += w[j];
    if (total_out) *total_out = total;
    const double target = u * total;
    double run = 0.0;
    int last = -1;
    for (int j = 0; j < count; ++j) {
        run += w[j];
        if (w[j] > 0.0) last = j;
        if (run > target && w[j] > 0.0) return j;
    }
    return last < 0 ? 0 : last;
}

}  // namespace qsv_channel_layout

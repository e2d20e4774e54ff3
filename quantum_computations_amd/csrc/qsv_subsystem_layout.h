// Host-side planning of the subsystem read-out (qsv_subsystem.hip): reduced states of up to 12 qubits
// left on the device, and marginal distributions of up to 26.  Plain C++ (tests/layout/subsystem_layout_driver.cpp
// compiles it stand-alone); the index functions are shared with the kernels, so the host test walks the same arithmetic.
//
// Vocabulary.  The caller's qubits[j] sits on physical bit cpos[j] of the flat index.  The KEPT positions, ascending, are
// kpos[0 .. kk): bit m of a ROW index is physical bit kpos[m].  The TRACED positions, ascending, are tpos[0 .. n - kk):
// bit m of a GROUP index is physical bit tpos[m].  l kept positions lie below 6 (lmask: which lane bits they are), h = kk - l
// at 6 and above.  A WAVE-LOAD is 64 consecutive amplitudes: its lanes carry the l low row bits (r_low) and the 6 - l low
// group bits (f_low); which load it is, is the pair (c_h = the h high row bits, w_hi = the high group bits).
//
// Reduced state, matrix-core form (k_subsys_tile).  The rows are cut into blocks of SUB_ROWS = 64; a block pair I <= J is
// a 64 x 64 piece of the upper triangle.  The groups are cut into tiles of SUB_TILE_GROUPS = 64 consecutive group indices,
// and the tiles into `slices` equal runs.  A work item is (block pair, slice): it owns every (row of I or J, group of the
// slice) and writes one 64 x 64 complex partial.  k_subsys_finish adds the partials of the slices in a fixed order,
// writes rho in the caller's order and mirrors it.  With fewer than six kept qubits the plan keeps `extra` traced
// positions as well (kk = 6), and the finishing kernel traces them out again.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SUB_HD __host__ __device__ inline
#else
#define SUB_HD inline
#endif

namespace qsv_subsystem_layout {

constexpr int SUB_BLOCK = 256;               // threads per workgroup (QSV_BLOCK)
constexpr int SUB_LANE_BITS = 6;
constexpr int SUB_MIN_QUBITS = 14;           // smaller registers take the per-entry forms (RO_MIN_QUBITS)
constexpr int SUB_MAX_K = 12;                // reduced state: 4096 x 4096 at most
constexpr int SUB_MARGINAL_MAX_K = 26;       // marginal: 2^26 doubles at most
constexpr int SUB_MAX_QUBITS = 40;           // what the position tables hold
constexpr int SUB_ROWS = 64;                 // B: rows of a block
constexpr int SUB_ROW_BITS = 6;
constexpr int SUB_TILE_GROUPS = 64;          // groups of a tile (what a work item owns at least)
constexpr int SUB_FILL_GROUPS = 32;          // groups staged in LDS at a time: two fills per tile
constexpr int SUB_PART_DOUBLES = 2 * SUB_ROWS * SUB_ROWS;   // one partial: 16 tile pairs x (re, im) x 256
constexpr uint32_t SUB_TARGET_ITEMS = 1024;  // slices are added until block pairs x slices reaches this
constexpr uint32_t SUB_MAX_ITEMS = 4096;     // and never beyond this: 4096 x 64 KiB = 256 MiB
constexpr uint64_t SUB_WORKSPACE_LIMIT = 256ull << 20;
constexpr uint32_t SUB_MARGINAL_WAVES = 4096;        // streaming marginal: waves (= partials) at most
constexpr uint64_t SUB_MARGINAL_PARTIALS = 1ull << 22;   // and waves x entries at most (32 MiB)

struct SubArgs {
    uint64_t W;                 // groups: 2^(n - kk)
    uint64_t tiles_per_slice;   // tiled form only
    uint32_t items, slices, nb; // tiled form: work items = pairs x slices, row blocks
    int32_t n, k, kk, extra;    // caller's k; kk = k + extra kept positions
    int32_t l, h;               // kept positions below / from bit 6
    uint32_t lmask;
    uint32_t kpos[SUB_MAX_K];           // 32-bit on purpose (qsv_device.h: dword arrays are read with scalar loads)
    uint32_t tpos[SUB_MAX_QUBITS];
    uint32_t cpos[SUB_MAX_K];           // physical bit of the caller's qubits[j]
    uint32_t rbit[SUB_MAX_K];           // row-index bit of the caller's qubits[j]
    uint32_t xbit[SUB_ROW_BITS];        // row-index bit of extra position m
};

struct MargArgs {
    uint64_t W;                 // groups: 2^(n - k)
    uint64_t run;               // streaming form: consecutive w_hi per wave and row setting
    uint32_t waves;             // streaming form: waves in the grid = partials
    int32_t n, k, l, h;
    uint32_t lmask;
    uint32_t kpos[SUB_MARGINAL_MAX_K];
    uint32_t tpos[SUB_MAX_QUBITS];
    uint32_t cpos[SUB_MARGINAL_MAX_K];
    uint32_t rbit[SUB_MARGINAL_MAX_K];
};

struct SubPlan {
    bool ok = false, tiled = false;
    SubArgs g;
    uint32_t grid = 0;          // k_subsys_tile (tiled) or k_subsys_entry
    uint32_t finish_grid = 0;   // k_subsys_finish
    uint64_t workspace_bytes = 0;
};

struct MargPlan {
    bool ok = false, streaming = false;
    MargArgs g;
    uint32_t grid = 0;
    uint64_t workspace_bytes = 0;   // partials (streaming) + the 2^k results
};

// ---- index functions shared by the kernels and the host model ------------------------------------------------------
template <class Args>
SUB_HD uint64_t sub_row_offset(const Args &g, uint32_t row, int kept) {   // physical-order row index -> address bits
    uint64_t off = 0;
    for (int m = 0; m < kept; ++m) off |= static_cast<uint64_t>((row >> m) & 1u) << g.kpos[m];
    return off;
}
template <class Args>
SUB_HD uint64_t sub_group_offset(const Args &g, uint64_t group, int first, int traced) {   // group bits first.. -> address bits
    uint64_t off = 0;
    for (int m = first; m < traced; ++m) off |= ((group >> m) & 1ull) << g.tpos[m];
    return off;
}
template <class Args>
SUB_HD uint64_t sub_caller_offset(const Args &g, uint64_t index) {       // caller-order index -> address bits
    uint64_t off = 0;
    for (int j = 0; j < g.k; ++j) off |= ((index >> (g.k - 1 - j)) & 1ull) << g.cpos[j];
    return off;
}
template <class Args>
SUB_HD uint32_t sub_caller_row(const Args &g, uint32_t index) {          // caller-order index -> physical-order row index
    uint32_t row = 0;
    for (int j = 0; j < g.k; ++j) row |= ((index >> (g.k - 1 - j)) & 1u) << g.rbit[j];
    return row;
}
SUB_HD uint32_t sub_extra_row(const SubArgs &g, uint32_t x) {
    uint32_t row = 0;
    for (int m = 0; m < g.extra; ++m) row |= ((x >> m) & 1u) << g.xbit[m];
    return row;
}
// first amplitude of the wave-load (w_hi, c_h): lane i of the wave reads this address + i
template <class Args>
SUB_HD uint64_t sub_load_base(const Args &g, uint64_t w_hi, uint32_t c_h, int kept, int traced) {
    const int fl = SUB_LANE_BITS - g.l;
    return sub_group_offset(g, w_hi << fl, fl, traced) | sub_row_offset(g, c_h << g.l, kept);
}
// the lane's place in a wave-load: row bits (kept bits < 6) and group bits (the other lane bits), each packed ascending
SUB_HD void sub_lane_place(uint32_t lmask, uint32_t lane, uint32_t *r_low, uint32_t *f_low) {
    uint32_t r = 0, f = 0;
    int rb = 0, fb = 0;
    for (int b = 0; b < SUB_LANE_BITS; ++b) {
        if ((lmask >> b) & 1u) r |= ((lane >> b) & 1u) << rb++;
        else f |= ((lane >> b) & 1u) << fb++;
    }
    *r_low = r;
    *f_low = f;
}
// k_subsys_tile stages 64 rows x 32 groups per block and fill; two fills (hf = 0, 1) make a tile of 64 groups.
// l > 0: 32 wave-loads, load j = (b, c_lo) with c_lo the fast index, every lane takes part.  l = 0: a load is one row and
// 64 groups, so there are 64 loads and the lanes whose group bit 5 equals hf take part.
SUB_HD uint32_t sub_fill_loads(int l) { return l ? 32u : 64u; }
struct SubLoad {
    uint64_t base;      // address of lane 0
    uint32_t row_hi;    // row within the block = row_hi | r_low
    uint32_t group_hi;  // group within the fill = (group_hi | f_low) & 31
};
SUB_HD SubLoad sub_tile_load(const SubArgs &g, uint64_t tile, uint32_t hf, uint32_t blk, uint32_t j) {
    const uint32_t l = static_cast<uint32_t>(g.l), fl = SUB_LANE_BITS - l;
    const uint32_t c_lo = j & ((1u << fl) - 1u), b = j >> fl;
    const uint64_t w_hi = l ? ((tile << l) | (static_cast<uint64_t>(hf) << (l - 1u)) | b) : tile;
    SubLoad out;
    out.base = sub_load_base(g, w_hi, (blk << fl) | c_lo, g.kk, g.n - g.kk);
    out.row_hi = c_lo << l;
    out.group_hi = b << fl;
    return out;
}
// The same load from its parts: the address bits of a load are an OR of what the tile, the block and the load itself
// contribute, so the kernel deposits the tile's bits once per tile (sub_tile_bits), the block's once per work item
// (sub_block_bits) and only the at most six group bits and six row bits of the load per load.
SUB_HD uint64_t sub_tile_bits(const SubArgs &g, uint64_t tile) { return sub_group_offset(g, tile << SUB_LANE_BITS, SUB_LANE_BITS, g.n - g.kk); }
SUB_HD uint64_t sub_block_bits(const SubArgs &g, uint32_t blk) { return sub_row_offset(g, blk << SUB_ROW_BITS, g.kk); }
SUB_HD SubLoad sub_tile_load_from(const SubArgs &g, uint64_t tile_bits, uint64_t block_bits, uint32_t hf, uint32_t j) {
    const uint32_t l = static_cast<uint32_t>(g.l), fl = SUB_LANE_BITS - l;
    const uint32_t c_lo = j & ((1u << fl) - 1u), b = j >> fl;
    const uint32_t w_lo = l ? ((hf << (l - 1u)) | b) : 0u;          // the low l bits of w_hi
    SubLoad out;
    out.base = tile_bits | block_bits | sub_group_offset(g, static_cast<uint64_t>(w_lo) << fl, static_cast<int>(fl), SUB_LANE_BITS) |
               sub_row_offset(g, c_lo << l, SUB_ROW_BITS);
    out.row_hi = c_lo << l;
    out.group_hi = b << fl;
    return out;
}
SUB_HD bool sub_lane_active(int l, uint32_t f_low, uint32_t hf) { return l != 0 || (f_low >> 5) == hf; }
// LDS slot (in amplitudes) of (side, row of the block, group of the fill): rows of 32 groups, the group index XORed with
// the row's low four bits so that the sixteen rows an MFMA operand reads fall into sixteen different 16-byte columns
SUB_HD uint32_t sub_lds_slot(uint32_t side, uint32_t row, uint32_t group) {
    return side * (SUB_ROWS * SUB_FILL_GROUPS) + row * SUB_FILL_GROUPS + (group ^ (row & 15u));
}
SUB_HD uint32_t sub_pair_index(uint32_t nb, uint32_t I, uint32_t J) { return I * nb - I * (I - 1u) / 2u + (J - I); }
SUB_HD void sub_pair_blocks(uint32_t nb, uint32_t pair, uint32_t *I, uint32_t *J) {
    uint32_t i = 0, rem = pair;
    while (rem >= nb - i) {
        rem -= nb - i;
        ++i;
    }
    *I = i;
    *J = i + rem;
}
// where entry (ip <= jp) of the physical-order matrix sits in a work item's partial: doubles from the partial's start
// (real part; the imaginary part follows 256 doubles later).  v_mfma_f64_16x16x4 leaves D[row][col] of a 16 x 16 tile in
// lane (row % 4) * 16 + col, register row / 4; the partial is [row tile of I][row tile of J][re, im][register][lane].
SUB_HD uint32_t sub_partial_slot(uint32_t ip, uint32_t jp) {
    const uint32_t ti = (ip >> 4) & 3u, tj = (jp >> 4) & 3u, row = ip & 15u, col = jp & 15u;
    return ((ti * 4u + tj) * 2u) * 256u + (row >> 2) * 64u + (row & 3u) * 16u + col;
}

// ---- plans ---------------------------------------------------------------------------------------------------------
inline uint32_t sub_pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p *= 2;
    return p;
}

// positions shared by both plans: kept (ascending), traced (ascending), row bits of the caller's legs
template <class Args>
inline void sub_fill_positions(Args &g, int n, int k, const int *bits, const uint64_t also_kept) {
    uint64_t kept = also_kept;
    for (int j = 0; j < k; ++j) kept |= 1ull << bits[j];
    int nk = 0, nt = 0;
    g.l = g.h = 0;
    g.lmask = 0;
    for (int b = 0; b < n; ++b) {
        if ((kept >> b) & 1ull) {
            for (int j = 0; j < k; ++j)
                if (bits[j] == b) g.rbit[j] = static_cast<uint32_t>(nk);
            g.kpos[nk++] = static_cast<uint32_t>(b);
            if (b < SUB_LANE_BITS) {
                ++g.l;
                g.lmask |= 1u << b;
            } else {
                ++g.h;
            }
        } else {
            g.tpos[nt++] = static_cast<uint32_t>(b);
        }
    }
    for (int j = 0; j < k; ++j) g.cpos[j] = static_cast<uint32_t>(bits[j]);
}

// bits[j] = physical bit of the caller's qubits[j] (distinct, below n); grid_cap > 0 limits the work-item grid
inline SubPlan sub_plan(int n, int k, const int *bits, int grid_cap) {
    SubPlan p;
    std::memset(&p.g, 0, sizeof(p.g));
    if (n < 1 || n > SUB_MAX_QUBITS || k < 1 || k > SUB_MAX_K || k > n) return p;
    SubArgs &g = p.g;
    g.n = n;
    g.k = k;
    const int kk = std::max(k, SUB_ROW_BITS);
    p.tiled = n >= SUB_MIN_QUBITS && n - kk >= SUB_LANE_BITS;   // at least one tile of 64 groups
    g.kk = p.tiled ? kk : k;
    g.extra = g.kk - k;
    uint64_t also = 0;
    {   // the extra positions: the lowest traced ones
        uint64_t kept = 0;
        for (int j = 0; j < k; ++j) kept |= 1ull << bits[j];
        int need = g.extra;
        for (int b = 0; b < n && need > 0; ++b)
            if (!((kept >> b) & 1ull)) {
                also |= 1ull << b;
                --need;
            }
    }
    sub_fill_positions(g, n, k, bits, also);
    for (int m = 0, x = 0; m < g.kk; ++m)
        if ((also >> g.kpos[m]) & 1ull) g.xbit[x++] = static_cast<uint32_t>(m);
    g.W = 1ull << (n - g.kk);
    const uint64_t D = 1ull << k;
    if (p.tiled) {
        g.nb = 1u << (g.kk - SUB_ROW_BITS);
        const uint32_t pairs = g.nb * (g.nb + 1u) / 2u;
        const uint64_t tiles = g.W / SUB_TILE_GROUPS;
        uint64_t slices = sub_pow2_at_least((SUB_TARGET_ITEMS + pairs - 1u) / pairs);
        while (slices > 1 && pairs * slices > SUB_MAX_ITEMS) slices /= 2;
        slices = std::min<uint64_t>(slices, tiles);
        g.slices = static_cast<uint32_t>(slices);
        g.tiles_per_slice = tiles / slices;
        g.items = pairs * g.slices;
        p.grid = grid_cap > 0 ? std::min<uint32_t>(g.items, static_cast<uint32_t>(grid_cap)) : g.items;
        p.workspace_bytes = sizeof(double) * SUB_PART_DOUBLES * static_cast<uint64_t>(g.items);
    } else {
        p.grid = static_cast<uint32_t>((D * D + SUB_BLOCK - 1) / SUB_BLOCK);
    }
    p.finish_grid = static_cast<uint32_t>((D * D + SUB_BLOCK - 1) / SUB_BLOCK);
    p.ok = true;
    return p;
}

inline MargPlan marginal_plan(int n, int k, const int *bits) {
    MargPlan p;
    std::memset(&p.g, 0, sizeof(p.g));
    if (n < 1 || n > SUB_MAX_QUBITS || k < 1 || k > SUB_MARGINAL_MAX_K || k > n) return p;
    MargArgs &g = p.g;
    g.n = n;
    g.k = k;
    sub_fill_positions(g, n, k, bits, 0);
    g.W = 1ull << (n - k);
    const uint64_t D = 1ull << k;
    const int w_bits = n - SUB_LANE_BITS - g.h;    // bits of w_hi
    p.streaming = n >= SUB_MIN_QUBITS && k <= SUB_MAX_K && w_bits >= SUB_LANE_BITS;
    if (p.streaming) {
        const uint64_t loads = 1ull << w_bits;
        const uint64_t waves = std::min<uint64_t>({loads, SUB_MARGINAL_WAVES, SUB_MARGINAL_PARTIALS >> k});
        g.waves = static_cast<uint32_t>(waves);
        g.run = loads / waves;
        p.grid = g.waves / (SUB_BLOCK / 64);
        p.workspace_bytes = sizeof(double) * (waves * D + D);
    } else {
        p.grid = static_cast<uint32_t>((D + SUB_BLOCK - 1) / SUB_BLOCK);
        p.workspace_bytes = sizeof(double) * D;
    }
    p.ok = true;
    return p;
}

}  // namespace qsv_subsystem_layout

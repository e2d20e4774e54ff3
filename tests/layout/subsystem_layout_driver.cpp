// TEST INFRASTRUCTURE: answers questions about qsv_subsystem_layout.h on the host (tests/test_subsystem_layout_host.py).
// One request per input line, one answer line each:
//   rdm n k cap b0 .. b(k-1)          (b_j = physical bit of the caller's qubits[j])
//     -> tiled kk extra l h lmask nb slices tiles_per_slice items grid finish_grid workspace W | kpos.. | tpos.. | rbit.. |
//        xbit.. | checked cover_min cover_max bad_addr bad_slot bad_range | entries write_min write_max bad_entry
//      The first check walks the loads as k_subsys_tile does (work item -> tile -> fill -> block -> wave-load -> lane) and
//      compares every address with a model written here from the caller's bits alone: the amplitude of (row of the block,
//      group of the tile).  cover_* count how often each (block side, row, group) of a walked tile is staged; bad_slot
//      counts LDS slots outside the tile or written twice in a fill.  Registers up to 2^16 amplitudes are walked whole
//      (every block pair, slice and tile); larger ones at sampled block pairs, the first and last slice and the first and
//      last two tiles of those.  The per-entry form is walked the same way: thread (i, j), group w.
//      The second check walks k_subsys_finish: every entry i <= j of the caller's matrix (k <= 9; sampled rows above)
//      must find, for every setting of the extra positions, a slot inside its block pair's partial whose physical rows
//      are the caller's rows; write_* count the writes to each entry of rho, mirror included.
//   marg n k b0 .. b(k-1)
//     -> streaming l h lmask waves run grid workspace W | kpos.. | tpos.. | rbit.. |
//        checked cover_min cover_max bad_addr bad_entry bad_range
//   slots -> sub_partial_slot(ip, jp) for ip, jp < 64, row-major
//   pairs nb -> for every pair index: I J, and sub_pair_index(I, J) must give the index back (else -1 -1)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_subsystem_layout.h"

using namespace qsv_subsystem_layout;

// the model: which physical bits are kept / traced, ascending, from the caller's bits alone
struct Model {
    std::vector<int> kept, traced;
};
static Model model_of(int n, uint64_t kept_mask) {
    Model m;
    for (int b = 0; b < n; ++b) ((kept_mask >> b) & 1ull ? m.kept : m.traced).push_back(b);
    return m;
}
static uint64_t spread(uint64_t index, const std::vector<int> &pos) {
    uint64_t out = 0;
    for (size_t i = 0; i < pos.size(); ++i) out |= ((index >> i) & 1ull) << pos[i];
    return out;
}
static uint64_t caller_addr(uint64_t index, int k, const int *bits) {
    uint64_t out = 0;
    for (int j = 0; j < k; ++j) out |= ((index >> (k - 1 - j)) & 1ull) << bits[j];
    return out;
}

struct Cover {
    uint64_t checked = 0, lo = ~0ull, hi = 0, bad_addr = 0, bad_slot = 0, bad_range = 0;
    void count(uint64_t c) {
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
};

template <class T>
static std::vector<T> sample(T count, T ends) {   // all of 0 .. count-1, or the first and last `ends`
    std::vector<T> out;
    for (T i = 0; i < count; ++i)
        if (count <= 2 * ends || i < ends || i >= count - ends) out.push_back(i);
    return out;
}

static void walk_tiled(const SubPlan &p, int n, const int *bits, Cover &c) {
    const SubArgs &g = p.g;
    uint64_t kept_mask = 0;
    for (int m = 0; m < g.kk; ++m) kept_mask |= 1ull << g.kpos[m];   // the plan's choice of extra positions is checked in Python
    const Model mod = model_of(n, kept_mask);
    const bool whole = n <= 16;
    const uint32_t pairs = g.nb * (g.nb + 1) / 2;
    std::vector<uint32_t> pair_list;
    if (whole || pairs <= 10) pair_list = sample<uint32_t>(pairs, pairs);
    else pair_list = {0u, 1u, g.nb - 1u, g.nb, pairs / 2u, pairs - 2u, pairs - 1u};
    for (uint32_t pair : pair_list) {
        uint32_t I, J;
        sub_pair_blocks(g.nb, pair, &I, &J);
        const uint32_t sides = I == J ? 1 : 2;
        for (uint32_t slice : whole ? sample<uint32_t>(g.slices, g.slices) : sample<uint32_t>(g.slices, 1)) {
            for (uint64_t tt : whole ? sample<uint64_t>(g.tiles_per_slice, g.tiles_per_slice) : sample<uint64_t>(g.tiles_per_slice, 2)) {
                const uint64_t t = slice * g.tiles_per_slice + tt;
                std::vector<int> staged(2 * SUB_ROWS * SUB_TILE_GROUPS, 0);
                for (uint32_t hf = 0; hf < 2; ++hf) {
                    std::vector<int> lds(2 * SUB_ROWS * SUB_FILL_GROUPS, 0);
                    for (uint32_t side = 0; side < sides; ++side)
                        for (uint32_t j = 0; j < sub_fill_loads(g.l); ++j) {
                            const SubLoad ld = sub_tile_load(g, t, hf, side ? J : I, j);
                            const SubLoad parts = sub_tile_load_from(g, sub_tile_bits(g, t), sub_block_bits(g, side ? J : I), hf, j);   // what the kernel calls
                            if (parts.base != ld.base || parts.row_hi != ld.row_hi || parts.group_hi != ld.group_hi) ++c.bad_addr;
                            for (uint32_t lane = 0; lane < 64; ++lane) {
                                uint32_t r_low, f_low;
                                sub_lane_place(g.lmask, lane, &r_low, &f_low);
                                if (!sub_lane_active(g.l, f_low, hf)) continue;
                                const uint32_t row = ld.row_hi | r_low, group = (ld.group_hi | f_low) & 31u;
                                const uint64_t addr = ld.base + lane;
                                ++c.checked;
                                if (addr >> n) ++c.bad_range;
                                const uint64_t g_row = static_cast<uint64_t>(side ? J : I) * SUB_ROWS + row;
                                const uint64_t g_group = t * SUB_TILE_GROUPS + hf * SUB_FILL_GROUPS + group;
                                if (row >= SUB_ROWS || addr != (spread(g_row, mod.kept) | spread(g_group, mod.traced))) ++c.bad_addr;
                                const uint32_t slot = sub_lds_slot(side, row, group);
                                if (slot >= lds.size() || lds[slot]++) ++c.bad_slot;
                                if (row < SUB_ROWS) ++staged[(side * SUB_ROWS + row) * SUB_TILE_GROUPS + hf * SUB_FILL_GROUPS + group];
                            }
                        }
                }
                for (size_t s = 0; s < sides * static_cast<size_t>(SUB_ROWS) * SUB_TILE_GROUPS; ++s) c.count(staged[s]);
            }
        }
    }
}

static void walk_entry(const SubPlan &p, int n, int k, const int *bits, Cover &c) {
    const SubArgs &g = p.g;
    uint64_t kept_mask = 0;
    for (int j = 0; j < k; ++j) kept_mask |= 1ull << bits[j];
    const Model mod = model_of(n, kept_mask);
    const uint64_t D = 1ull << k;
    const bool whole = n <= 18;
    std::vector<uint8_t> seen(whole ? (1ull << n) : 0, 0);
    for (uint64_t i : whole ? sample<uint64_t>(D, D) : sample<uint64_t>(D, 2))
        for (uint64_t w : whole ? sample<uint64_t>(g.W, g.W) : sample<uint64_t>(g.W, 2)) {
            const uint64_t addr = sub_group_offset(g, w, 0, n - k) + sub_caller_offset(g, i);
            ++c.checked;
            if (addr >> n) {
                ++c.bad_range;
                continue;
            }
            if (addr != (caller_addr(i, k, bits) | spread(w, mod.traced))) ++c.bad_addr;
            if (whole) ++seen[addr];
        }
    if (whole)
        for (uint8_t s : seen) c.count(s);
    else
        c.count(1);
}

struct Finish {
    uint64_t entries = 0, lo = ~0ull, hi = 0, bad = 0;
};
static void walk_finish(const SubPlan &p, int n, int k, const int *bits, Finish &f) {
    const SubArgs &g = p.g;
    const uint64_t D = 1ull << k;
    const bool whole = k <= 9;
    std::vector<uint8_t> written(whole ? D * D : 0, 0);
    uint64_t kept_mask = 0;
    for (int m = 0; m < g.kk; ++m) kept_mask |= 1ull << g.kpos[m];
    const Model mod = model_of(n, kept_mask);
    std::vector<int> extra_pos;
    for (int m = 0; m < g.extra; ++m) extra_pos.push_back(static_cast<int>(g.kpos[g.xbit[m]]));
    const uint32_t pairs = g.nb * (g.nb + 1) / 2;
    for (uint64_t ic : whole ? sample<uint64_t>(D, D) : sample<uint64_t>(D, 3))
        for (uint64_t jc = ic; jc < D; ++jc) {
            ++f.entries;
            if (p.tiled)
                for (uint32_t x = 0; x < (1u << g.extra); ++x) {
                    const uint32_t x_row = sub_extra_row(g, x);
                    uint32_t ip = sub_caller_row(g, static_cast<uint32_t>(ic)) | x_row, jp = sub_caller_row(g, static_cast<uint32_t>(jc)) | x_row;
                    const uint64_t xa = spread(x, extra_pos);
                    if (spread(ip, mod.kept) != (caller_addr(ic, k, bits) | xa) || spread(jp, mod.kept) != (caller_addr(jc, k, bits) | xa)) ++f.bad;
                    if (ip > jp) std::swap(ip, jp);
                    const uint32_t pair = sub_pair_index(g.nb, ip >> SUB_ROW_BITS, jp >> SUB_ROW_BITS);
                    uint32_t I, J;
                    sub_pair_blocks(g.nb, pair, &I, &J);
                    if (pair >= pairs || I != (ip >> SUB_ROW_BITS) || J != (jp >> SUB_ROW_BITS)) ++f.bad;
                    if (sub_partial_slot(ip, jp) + 256u >= static_cast<uint32_t>(SUB_PART_DOUBLES)) ++f.bad;
                }
            if (whole) {
                ++written[ic * D + jc];
                if (ic != jc) ++written[jc * D + ic];
            }
        }
    if (whole)
        for (uint8_t w : written) {
            f.lo = w < f.lo ? w : f.lo;
            f.hi = w > f.hi ? w : f.hi;
        }
    else
        f.lo = f.hi = 1;
}

static void walk_marginal(const MargPlan &p, int n, int k, const int *bits, Cover &c) {
    const MargArgs &g = p.g;
    uint64_t kept_mask = 0;
    for (int j = 0; j < k; ++j) kept_mask |= 1ull << bits[j];
    const Model mod = model_of(n, kept_mask);
    const uint64_t D = 1ull << k;
    const bool whole = n <= 18;
    std::vector<uint8_t> seen(whole ? (1ull << n) : 0, 0);
    if (p.streaming) {
        const uint32_t traced_lanes = ~g.lmask & 63u;
        const int fl = SUB_LANE_BITS - g.l;
        for (uint32_t wave : whole ? sample<uint32_t>(g.waves, g.waves) : sample<uint32_t>(g.waves, 2))
            for (uint32_t c_h : whole ? sample<uint32_t>(1u << g.h, 1u << g.h) : sample<uint32_t>(1u << g.h, 2))
                for (uint64_t q : whole ? sample<uint64_t>(g.run, g.run) : sample<uint64_t>(g.run, 2)) {
                    const uint64_t w_hi = wave * g.run + q, base = sub_load_base(g, w_hi, c_h, k, n - k);
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        uint32_t r_low, f_low;
                        sub_lane_place(g.lmask, lane, &r_low, &f_low);
                        const uint64_t row = (static_cast<uint64_t>(c_h) << g.l) | r_low, addr = base + lane;
                        ++c.checked;
                        if (addr >> n) {
                            ++c.bad_range;
                            continue;
                        }
                        if (addr != (spread(row, mod.kept) | spread((w_hi << fl) | f_low, mod.traced))) ++c.bad_addr;
                        if (row >= D || ((lane & traced_lanes) == 0) != (f_low == 0)) ++c.bad_slot;   // the lane that writes the row's sum
                        if (whole) ++seen[addr];
                    }
                }
    } else {
        for (uint64_t i : whole ? sample<uint64_t>(D, D) : sample<uint64_t>(D, 2))
            for (uint64_t w : whole ? sample<uint64_t>(g.W, g.W) : sample<uint64_t>(g.W, 2)) {
                const uint64_t addr = sub_caller_offset(g, i) + sub_group_offset(g, w, 0, n - k);
                ++c.checked;
                if (addr >> n) {
                    ++c.bad_range;
                    continue;
                }
                if (addr != (caller_addr(i, k, bits) | spread(w, mod.traced))) ++c.bad_addr;
                if (whole) ++seen[addr];
            }
    }
    if (whole)
        for (uint8_t s : seen) c.count(s);
    else
        c.count(1);
}

template <class T>
static void print_list(const T *v, int count) {
    std::printf(" |");
    for (int i = 0; i < count; ++i) std::printf(" %u", static_cast<unsigned>(v[i]));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "rdm") {
            int n, k, cap, bits[SUB_MAX_K] = {0};
            in >> n >> k >> cap;
            for (int j = 0; j < k && j < SUB_MAX_K; ++j) in >> bits[j];
            const SubPlan p = sub_plan(n, k, bits, cap);
            if (!p.ok) {
                std::printf("-1\n");
                continue;
            }
            const SubArgs &g = p.g;
            std::printf("%d %d %d %d %d %u %u %u %" PRIu64 " %u %u %u %" PRIu64 " %" PRIu64, p.tiled ? 1 : 0, g.kk, g.extra, g.l, g.h, g.lmask,
                        g.nb, g.slices, g.tiles_per_slice, g.items, p.grid, p.finish_grid, p.workspace_bytes, g.W);
            print_list(g.kpos, g.kk);
            print_list(g.tpos, n - g.kk);
            print_list(g.rbit, k);
            print_list(g.xbit, g.extra);
            Cover c;
            if (p.tiled) walk_tiled(p, n, bits, c);
            else walk_entry(p, n, k, bits, c);
            std::printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, c.checked, c.lo, c.hi, c.bad_addr, c.bad_slot, c.bad_range);
            Finish f;
            walk_finish(p, n, k, bits, f);
            std::printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", f.entries, f.lo, f.hi, f.bad);
        } else if (what == "marg") {
            int n, k, bits[SUB_MARGINAL_MAX_K] = {0};
            in >> n >> k;
            for (int j = 0; j < k && j < SUB_MARGINAL_MAX_K; ++j) in >> bits[j];
            const MargPlan p = marginal_plan(n, k, bits);
            if (!p.ok) {
                std::printf("-1\n");
                continue;
            }
            const MargArgs &g = p.g;
            std::printf("%d %d %d %u %u %" PRIu64 " %u %" PRIu64 " %" PRIu64, p.streaming ? 1 : 0, g.l, g.h, g.lmask, g.waves, g.run, p.grid,
                        p.workspace_bytes, g.W);
            print_list(g.kpos, k);
            print_list(g.tpos, n - k);
            print_list(g.rbit, k);
            Cover c;
            walk_marginal(p, n, k, bits, c);
            std::printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c.checked, c.lo, c.hi, c.bad_addr, c.bad_slot, c.bad_range);
        } else if (what == "slots") {
            for (uint32_t ip = 0; ip < 64; ++ip)
                for (uint32_t jp = 0; jp < 64; ++jp) std::printf("%u ", sub_partial_slot(ip, jp));
            std::printf("\n");
        } else if (what == "pairs") {
            uint32_t nb;
            in >> nb;
            for (uint32_t pair = 0; pair < nb * (nb + 1) / 2; ++pair) {
                uint32_t I, J;
                sub_pair_blocks(nb, pair, &I, &J);
                if (I <= J && J < nb && sub_pair_index(nb, I, J) == pair) std::printf("%u %u ", I, J);
                else std::printf("-1 -1 ");
            }
            std::printf("\n");
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}

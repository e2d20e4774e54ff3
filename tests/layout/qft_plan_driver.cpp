// TEST INFRASTRUCTURE: text front end of the pass planner of qsv_apply_qft (csrc/qsv_qft_plan.h), driven by
// tests/test_qft_plan_host.py under AddressSanitizer + UBSan.
//
// One request per line:   <n> <flags> <m> <bit_0> ... <bit_{m-1}> <k> <index_1> ... <index_k>      (indices in decimal)
// One answer per line:    <passes>, then per pass
//     <tile_bits> <n_stages> <twiddle_first> <conj_twiddle> <scale as a hexadecimal float>   <pos> x tile_bits
//     per stage:  <rank> <tile_index> <L> <run> <reg> <n_later> (<in tile> <tile index | index bit> <shift>) x n_later
//     <n_runs>  per run: <first> <count> <q> x min(4, tile_bits)
//     per index: qft_turns(index, pass, stage) x n_stages
// The later list of a stage is read off the pass's split of X (in_shift / out_shift) below the stage's mask; qft_turns is
// also compared here with the same sum over that list, so the split and the statement cannot drift apart.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_qft_plan.h"

int main() {
    namespace plan = qsv_qft_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int n = 0, flags = 0, m = 0;
        if (!(in >> n >> flags >> m) || m < 0 || m > plan::MAX_QUBITS) return 2;
        std::vector<int> bits(m);
        for (int &b : bits)
            if (!(in >> b)) return 2;
        size_t k = 0;
        if (!(in >> k)) return 2;
        std::vector<uint64_t> indices(k);
        for (uint64_t &i : indices)
            if (!(in >> i)) return 2;
        const std::vector<plan::Pass> passes = plan::qft_plan(n, bits, flags);
        std::printf("%zu", passes.size());
        for (const plan::Pass &p : passes) {
            std::printf(" %d %d %d %d %a", p.tile_bits, p.n_stages, p.twiddle_first, p.conj_twiddle, p.scale);
            for (int j = 0; j < p.tile_bits; ++j) std::printf(" %u", p.pos[j]);
            struct Later {
                int in_tile, where, shift;
            };
            std::vector<std::vector<Later>> later(p.n_stages);
            for (int s = 0; s < p.n_stages; ++s) {
                for (int j = 0; j < p.tile_bits; ++j)
                    if (p.in_shift[j] >= 0 && p.in_shift[j] < p.L[s] - 1) later[s].push_back({1, j, p.in_shift[j]});
                for (int i = 0; i < p.n_out; ++i)
                    if (p.out_shift[i] < p.L[s] - 1) later[s].push_back({0, p.out_bit[i], p.out_shift[i]});
                std::printf(" %d %d %d %d %d %zu", p.rank[s], p.tile_index[s], p.L[s], p.run[s], p.reg[s], later[s].size());
                for (const Later &l : later[s]) std::printf(" %d %d %d", l.in_tile, l.where, l.shift);
            }
            std::printf(" %d", p.n_runs);
            for (int u = 0; u < p.n_runs; ++u) {
                std::printf(" %d %d", p.run_first[u], p.run_count[u]);
                for (int j = 0; j < std::min(plan::RUN_BITS, p.tile_bits); ++j) std::printf(" %d", p.run_q[u][j]);
            }
            for (uint64_t index : indices)
                for (int s = 0; s < p.n_stages; ++s) {
                    const uint64_t turns = plan::qft_turns(index, p, s);
                    uint64_t listed = 0;
                    for (const Later &l : later[s]) listed |= ((index >> (l.in_tile ? p.pos[l.where] : l.where)) & 1ull) << l.shift;
                    if (listed != turns) return 3;
                    // the kernel's split: the register bits of the stage's run (its table) and the rest of the tile (the thread)
                    const uint32_t t = plan::qft_tile_index(index, p);
                    uint32_t reg_mask = 0;
                    for (int j = 0; j < std::min(plan::RUN_BITS, p.tile_bits); ++j) reg_mask |= 1u << p.run_q[p.run[s]][j];
                    uint64_t table = 0;
                    int other = 0;
                    for (int j = 0; j < std::min(plan::RUN_BITS, p.tile_bits); ++j) {
                        const int q = p.run_q[p.run[s]][j];
                        if (j == p.reg[s]) continue;
                        const int shift = p.reg_shift[s][other++];
                        if (((t >> q) & 1u) && shift >= 0) table |= 1ull << shift;
                    }
                    const uint64_t thread = plan::qft_turns_out(index, p) | plan::qft_turns_in(t & ~reg_mask, p);
                    if (((thread | table) & plan::qft_turns_mask(p.L[s])) != turns) return 4;
                    std::printf(" %" PRIu64, turns);
                }
        }
        std::printf("\n");
    }
    return 0;
}

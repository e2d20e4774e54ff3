// TEST INFRASTRUCTURE: text front end of the pass planner of qsv_apply_layer (csrc/qsv_layer_plan.h), driven by
// tests/test_layer_plan_host.py under AddressSanitizer + UBSan.
//
// One request per line:   <n> <b> <k> <bit_0> ... <bit_{k-1}>          (n: bits of a member, b: log2 of the members)
// One answer per line:    <passes> <layer_passes> <table_doubles>  <order> x k, then per pass
//     <tile_bits> <n_stages> <first>   <pos> x tile_bits
//     per stage:  <bit> <tile_index> <run> <reg> <table_offset of the first and of the last member>
//     <n_runs>  per run: <first> <count> <q> x min(4, tile_bits)
//     <pairs_ok>: 1 if, for every stage, both amplitudes of the first, the last and a middle pair of a member lie in the member
// The plan is made from n and the bits alone; b enters the table's size and the last member's offsets only, which the test
// checks by asking for the same layer with several b.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_layer_plan.h"

int main() {
    namespace plan = qsv_layer_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int n = 0, b = 0, k = 0;
        if (!(in >> n >> b >> k) || n < 1 || b < 0 || n + b >= plan::MAX_QUBITS || k < 0 || k > n) return 2;
        std::vector<int> bits(k);
        for (int &x : bits)
            if (!(in >> x) || x < 0 || x >= n) return 2;
        const uint64_t members = 1ull << b;
        const plan::Layer layer = plan::layer_plan(n, bits);
        std::printf("%zu %" PRIu64 " %" PRIu64, layer.passes.size(), plan::layer_passes(n, bits), plan::table_doubles(members, k));
        for (int s = 0; s < k; ++s) std::printf(" %d", layer.order[s]);
        for (const plan::Pass &p : layer.passes) {
            std::printf(" %d %d %d", p.tile_bits, p.n_stages, p.first);
            for (int j = 0; j < p.tile_bits; ++j) std::printf(" %u", p.pos[j]);
            bool pairs_ok = true;
            for (int s = 0; s < p.n_stages; ++s) {
                std::printf(" %d %d %d %d %" PRIu64 " %" PRIu64, p.bit[s], p.tile_index[s], p.run[s], p.reg[s], plan::table_offset(0, k, p.first + s),
                            plan::table_offset(members - 1, k, p.first + s));
                const uint64_t pairs = 1ull << (n - 1);
                for (uint64_t w : {uint64_t{0}, pairs / 2, pairs - 1, pairs / 3}) {
                    const uint64_t lo = plan::pair_low(w, p.bit[s]), hi = plan::pair_high(w, p.bit[s]);
                    if ((lo >> n) != 0 || (hi >> n) != 0 || hi != (lo | (1ull << p.bit[s])) || ((lo >> p.bit[s]) & 1ull)) pairs_ok = false;
                }
            }
            std::printf(" %d", p.n_runs);
            for (int u = 0; u < p.n_runs; ++u) {
                std::printf(" %d %d", p.run_first[u], p.run_count[u]);
                for (int j = 0; j < std::min(plan::RUN_BITS, p.tile_bits); ++j) std::printf(" %d", p.run_q[u][j]);
            }
            std::printf(" %d", pairs_ok ? 1 : 0);
        }
        std::printf("\n");
    }
    return 0;
}

// TEST INFRASTRUCTURE: answers questions about quantum_computations_amd/csrc/qsv_krylov_layout.h on the host
// (tests/test_krylov_layout_host.py).  One request per line on stdin, one answer line per request on stdout; parts of an
// answer are separated by '|', doubles are printed as hex floats.
//   grids <amps> <grid_cap>                                       -> reduce_grid stream_grid
//   lincomb <n_src> <beta_re> <beta_im> <norm> <amps> <grid_cap>  -> per pass: first count beta_re beta_im reads_dst norm grid offset
//                                                                    c_re[8] c_im[8] src[8] (coefficient k = (k + 1, -(k + 1)), source k at 4096 (k + 1))
//   inner <n_x> <amps> <grid_cap>                                 -> doubles | per pass: first count grid offset x[8] (x_k at 4096 (k + 1))
//   innersum <n_x> <amps> <grid_cap> <doubles...>                 -> values (2 n_x)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_krylov_layout.h"

using namespace qsv_krylov_layout;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "grids") {
            uint64_t amps;
            int cap;
            in >> amps >> cap;
            std::printf("%d %d\n", reduce_grid(amps, cap), stream_grid(amps, cap));
        } else if (what == "lincomb") {
            int n_src, norm, cap;
            double beta_re, beta_im;
            uint64_t amps;
            in >> n_src >> beta_re >> beta_im >> norm >> amps >> cap;
            std::vector<double> coeffs(2 * static_cast<size_t>(n_src));      // exactly n_src entries: ASan sees a read past them
            std::vector<const void *> srcs(n_src);
            for (int k = 0; k < n_src; ++k) {
                coeffs[2 * k] = k + 1;
                coeffs[2 * k + 1] = -(k + 1);
                srcs[k] = reinterpret_cast<const void *>(static_cast<uintptr_t>(4096) * (k + 1));
            }
            const std::vector<LincombPass> plan = lincomb_passes(n_src, beta_re, beta_im, norm != 0, amps, cap);
            for (size_t p = 0; p < plan.size(); ++p) {
                const LincombPass &a = plan[p];
                const LincombArgs g = lincomb_args(a, amps, coeffs.data(), srcs.data());
                std::printf("%s%d %d %a %a %d %d %d %zu", p ? " | " : "", a.first, a.count, g.beta_re, g.beta_im, int(a.reads_dst), int(a.norm), a.grid,
                            a.partial_offset);
                for (int k = 0; k < KRYLOV_OPERANDS_PER_PASS; ++k) std::printf(" %a", g.c_re[k]);
                for (int k = 0; k < KRYLOV_OPERANDS_PER_PASS; ++k) std::printf(" %a", g.c_im[k]);
                for (int k = 0; k < KRYLOV_OPERANDS_PER_PASS; ++k) std::printf(" %llu", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(g.src[k])));
                if (g.amps != amps) std::printf(" BAD");
            }
            std::printf("\n");
        } else if (what == "inner" || what == "innersum") {
            int n_x, cap;
            uint64_t amps;
            in >> n_x >> amps >> cap;
            std::vector<const void *> xs(n_x);
            for (int k = 0; k < n_x; ++k) xs[k] = reinterpret_cast<const void *>(static_cast<uintptr_t>(4096) * (k + 1));
            const InnerPlan plan = inner_plan(n_x, amps, cap);
            if (what == "inner") {
                std::printf("%zu", plan.doubles);
                for (const InnerPass &a : plan.passes) {
                    const InnerManyArgs g = inner_args(a, amps, xs.data());
                    std::printf(" | %d %d %d %zu", a.first, a.count, a.grid, a.partial_offset);
                    for (int k = 0; k < KRYLOV_OPERANDS_PER_PASS; ++k) std::printf(" %llu", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(g.x[k])));
                    if (g.amps != amps) std::printf(" BAD");
                }
                std::printf("\n");
            } else {
                std::vector<double> host(plan.doubles), values(2 * static_cast<size_t>(n_x));
                for (double &v : host) in >> v;
                for (const InnerPass &a : plan.passes) inner_sum(a, host.data(), values.data());
                for (size_t k = 0; k < values.size(); ++k) std::printf("%s%a", k ? " " : "", values[k]);
                std::printf("\n");
            }
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}

// TEST INFRASTRUCTURE: text front end of the pass planner of qsv_expect_pauli_sum (csrc/qsv_pauli_plan.h), driven by
// tests/test_pauli_plan_host.py under AddressSanitizer + UBSan.
//
// One request per line:   <n_terms> <xmask> <zmask> <xmask> <zmask> ...      (masks in hex)
// One answer per line:    <PAULI_TERMS_PER_PASS> <passes> | <xmask> <pivot> <zmask> <nY> <index> <scale> ... | ...
// with one '|' part per pass and four tokens per term of the pass; scale is pair_scale(pivot, nY).
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_pauli_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        size_t n_terms = 0;
        if (!(in >> n_terms)) return 2;
        std::vector<qsv_pauli_plan::Term> terms(n_terms);
        in >> std::hex;
        for (qsv_pauli_plan::Term &t : terms)
            if (!(in >> t.xmask >> t.zmask)) return 2;
        const std::vector<qsv_pauli_plan::Pass> passes = qsv_pauli_plan::plan(terms);
        std::printf("%d %zu", qsv_pauli_plan::PAULI_TERMS_PER_PASS, passes.size());
        for (const qsv_pauli_plan::Pass &p : passes) {
            if (p.zmask.size() != p.n_y.size() || p.zmask.size() != p.index.size()) return 3;
            std::printf(" | %" PRIx64 " %d", p.xmask, p.pivot);
            for (size_t t = 0; t < p.zmask.size(); ++t)
                std::printf(" %" PRIx64 " %d %d %d", p.zmask[t], p.n_y[t], p.index[t],
                            static_cast<int>(qsv_pauli_plan::pair_scale(p.pivot, p.n_y[t])));
        }
        std::printf("\n");
    }
    return 0;
}

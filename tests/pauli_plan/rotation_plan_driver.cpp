// TEST INFRASTRUCTURE: text front end of the pass planner of qsv_apply_pauli_rotations
// (csrc/qsv_pauli_rotation_plan.h), driven by tests/test_pauli_rotation_plan_host.py under AddressSanitizer + UBSan.
//
// One request per line:   <n_terms> <xmask> <zmask> <xmask> <zmask> ...      (masks in hex)
// One answer per line:    <ROTATIONS_PER_PASS> <passes> | <xmask> <pivot> <index> <term xmask> <zmask> <nY> ... | ...
// with one '|' part per pass and four tokens per term of the pass.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_pauli_rotation_plan.h"

int main() {
    namespace plan = qsv_pauli_rotation_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        size_t n_terms = 0;
        if (!(in >> n_terms)) return 2;
        std::vector<plan::Term> terms(n_terms);
        in >> std::hex;
        for (plan::Term &t : terms)
            if (!(in >> t.xmask >> t.zmask)) return 2;
        const std::vector<plan::Pass> passes = plan::plan(terms);
        std::printf("%d %zu", plan::ROTATIONS_PER_PASS, passes.size());
        for (const plan::Pass &p : passes) {
            const size_t count = p.index.size();
            if (p.term_xmask.size() != count || p.zmask.size() != count || p.n_y.size() != count) return 3;
            std::printf(" | %" PRIx64 " %d", p.xmask, p.pivot);
            for (size_t t = 0; t < count; ++t)
                std::printf(" %d %" PRIx64 " %" PRIx64 " %d", p.index[t], p.term_xmask[t], p.zmask[t], p.n_y[t]);
        }
        std::printf("\n");
    }
    return 0;
}

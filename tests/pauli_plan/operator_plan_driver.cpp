// TEST INFRASTRUCTURE: text front end of the argument builders of qsv_apply_pauli_sum and qsv_pauli_rotations_adjoint
// (pauli_sum_apply_passes / pauli_adjoint_passes in csrc/qsv_readout_layout.h, on the plans of csrc/qsv_pauli_plan.h and
// csrc/qsv_pauli_rotation_plan.h), driven by tests/test_pauli_operator_plan_host.py under AddressSanitizer + UBSan.
//
// One request per line (masks and sizes in hex, doubles as hex floats):
//     S <amps> <accumulate> <n_terms> { <xmask> <zmask> <c re> <c im> } ...
//     A <amps> <n_terms> { <xmask> <zmask> <cos> <sin> } ...
// One answer per line, one '|' part per launch:
//     S: <launches> | <ok> <xmask> <pivot> <items> <odd> <width> <first> { <zmask> <d re> <d im> } x 8
//     A: <launches> | <ok> <xmask> <pivot> <items> <diag> <rot> <width> { <index> <nY> <zmask> <cos> <sin> } x 8
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_readout_layout.h"

static bool read_double(std::istringstream &in, double *out) {
    std::string token;
    if (!(in >> token)) return false;
    return std::sscanf(token.c_str(), "%la", out) == 1;
}

int main() {
    namespace layout = qsv_readout_layout;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        uint64_t amps = 0;
        int accumulate = 0;
        size_t n_terms = 0;
        if (!(in >> kind >> std::hex >> amps >> std::dec)) return 2;
        if (kind == "S" && !(in >> accumulate)) return 2;
        if (!(in >> n_terms)) return 2;
        std::vector<qsv_pauli_plan::Term> terms(n_terms);
        std::vector<double> first(n_terms), second(n_terms);
        for (size_t t = 0; t < n_terms; ++t) {
            if (!(in >> std::hex >> terms[t].xmask >> terms[t].zmask >> std::dec)) return 2;
            if (!read_double(in, &first[t]) || !read_double(in, &second[t])) return 2;
        }
        if (kind == "S") {
            std::vector<double> coeffs(2 * n_terms);
            for (size_t t = 0; t < n_terms; ++t) {
                coeffs[2 * t] = first[t];
                coeffs[2 * t + 1] = second[t];
            }
            const std::vector<layout::PauliSumApply> launches = layout::pauli_sum_apply_passes(qsv_pauli_plan::plan(terms), amps, coeffs.data(), accumulate != 0);
            std::printf("%zu", launches.size());
            for (const layout::PauliSumApply &a : launches) {
                std::printf(" | %d %" PRIx64 " %d %" PRIx64 " %x %d %d", a.ok ? 1 : 0, a.g.xmask, a.g.pivot, a.g.items, a.g.odd, a.width, a.first ? 1 : 0);
                for (int t = 0; t < qsv_pauli_plan::PAULI_TERMS_PER_PASS; ++t) std::printf(" %" PRIx64 " %a %a", a.g.zmask[t], a.g.d_re[t], a.g.d_im[t]);
            }
        } else if (kind == "A") {
            const std::vector<layout::PauliAdjoint> walk = layout::pauli_adjoint_passes(qsv_pauli_rotation_plan::plan(terms), amps, first.data(), second.data());
            std::printf("%zu", walk.size());
            for (const layout::PauliAdjoint &a : walk) {
                const layout::PauliRotateArgs &g = a.r.g;
                std::printf(" | %d %" PRIx64 " %d %" PRIx64 " %x %x %d", a.r.ok ? 1 : 0, g.xmask, g.pivot, g.items, g.diag, g.rot, a.r.width);
                for (int t = 0; t < qsv_pauli_rotation_plan::ROTATIONS_PER_PASS; ++t)
                    std::printf(" %d %d %" PRIx64 " %a %a", a.index[t], a.n_y[t], g.zmask[t], g.cs[t], g.sn[t]);
            }
        } else {
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}

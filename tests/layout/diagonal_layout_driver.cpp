// TEST INFRASTRUCTURE: answers questions about quantum_computations_amd/csrc/qsv_diagonal_layout.h on the host
// (tests/test_diagonal_layout_host.py).  One request per line on stdin, one answer line per request on stdout; parts of an
// answer are separated by '|', doubles are printed as hex floats.
//   pack <n> <coeffs 0/1> <T> then T terms "<letters or ->:<q,q,...>:<coeff>"  -> error | per term: zmask coeff
//   value <n> <start> <i> <T> terms...                                         -> table_value(i) (start added first)
//   grids <items> <grid_cap>                                                   -> reduce_grid stream_grid
//   slices <items> <grid_cap> <slots>                                          -> grid words bytes | every partial_index in (block, slot) order
//   sums <items> <grid_cap> <slots> <doubles...>                               -> reduce_sums
//   extrema <items> <grid_cap> then per block "min argmin max argmax"          -> min argmin max argmax
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_diagonal_layout.h"

using namespace qsv_diagonal_layout;

struct Flat {
    std::vector<int> offsets{0}, qubits;
    std::string letters;
    std::vector<double> coeffs;
};

static Flat read_terms(std::istringstream &in, int count) {
    Flat f;
    for (int t = 0; t < count; ++t) {
        std::string token;
        in >> token;
        const size_t a = token.find(':'), b = token.find(':', a + 1);
        const std::string letters = token.substr(0, a), qs = token.substr(a + 1, b - a - 1);
        if (letters != "-") f.letters += letters;
        std::istringstream list(qs);
        std::string q;
        while (std::getline(list, q, ','))
            if (!q.empty()) f.qubits.push_back(std::stoi(q));
        f.offsets.push_back(static_cast<int>(f.qubits.size()));
        f.coeffs.push_back(std::stod(token.substr(b + 1)));
    }
    return f;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "pack" || what == "value") {
            int n, with_coeffs = 1, count;
            double start = 0.0;
            unsigned long long index = 0;
            in >> n;
            if (what == "pack")
                in >> with_coeffs;
            else
                in >> start >> index;
            in >> count;
            // exactly as many entries as the caller's arrays hold: ASan sees a read past them
            const Flat f = read_terms(in, count);
            std::vector<int> qubits(f.qubits);
            std::vector<char> letters(f.letters.begin(), f.letters.end());
            std::vector<DiagTerm> rows(3, DiagTerm{77, 7.0});
            const PackError e = pack_terms(n, count, f.offsets.data(), qubits.empty() ? nullptr : qubits.data(),
                                           letters.empty() ? nullptr : letters.data(), with_coeffs ? f.coeffs.data() : nullptr, &rows);
            if (what == "value") {
                std::printf("%a\n", e == PACK_OK ? table_value(rows.data(), rows.size(), index, start) : 0.0 / 0.0);
                continue;
            }
            std::printf("%d", static_cast<int>(e));
            if (e != PACK_OK && !(rows.size() == 3 && rows[0].zmask == 77)) std::printf(" TOUCHED");
            if (e == PACK_OK)
                for (const DiagTerm &r : rows) std::printf(" | %llu %a", static_cast<unsigned long long>(r.zmask), r.coeff);
            std::printf("\n");
        } else if (what == "grids") {
            uint64_t items;
            int cap;
            in >> items >> cap;
            std::printf("%d %d\n", reduce_grid(items, cap), stream_grid(items, cap));
        } else if (what == "slices" || what == "sums") {
            uint64_t items;
            int cap, slots;
            in >> items >> cap >> slots;
            const ReducePlan p = reduce_plan(items, cap, slots);
            if (what == "slices") {
                std::printf("%d %zu %zu |", p.grid, p.words, p.bytes);
                for (int b = 0; b < p.grid; ++b)
                    for (int s = 0; s < slots; ++s) std::printf(" %zu", partial_index(p, b, s));
                std::printf("\n");
            } else {
                std::vector<double> host(p.words), out(slots);
                for (double &v : host) in >> v;
                reduce_sums(p, host.data(), out.data());
                for (int s = 0; s < slots; ++s) std::printf("%s%a", s ? " " : "", out[s]);
                std::printf("\n");
            }
        } else if (what == "extrema") {
            uint64_t items;
            int cap;
            in >> items >> cap;
            const ReducePlan p = reduce_plan(items, cap, EXTREMA_SLOTS);
            std::vector<uint64_t> words(p.words);
            for (int b = 0; b < p.grid; ++b) {
                double mn, mx;
                unsigned long long amn, amx;
                in >> mn >> amn >> mx >> amx;
                std::memcpy(&words[partial_index(p, b, 0)], &mn, 8);
                words[partial_index(p, b, 1)] = amn;
                std::memcpy(&words[partial_index(p, b, 2)], &mx, 8);
                words[partial_index(p, b, 3)] = amx;
            }
            const Extrema e = reduce_extrema(p, words.data());
            std::printf("%a %llu %a %llu\n", e.min, static_cast<unsigned long long>(e.argmin), e.max, static_cast<unsigned long long>(e.argmax));
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}

// TEST INFRASTRUCTURE: answers questions about qsv_split_rules.h and the pair schedule of qsv_jacobi.h on the host
// (tests/test_split_rules_host.py).  One request per input line, one answer line each; doubles go in as decimals that
// round-trip (or "inf"), and come back as hexadecimal floats.  "v.." is a count followed by that many doubles.
//   schedule lp                                   -> p q of every pair, step by step (lp - 1 steps of lp / 2 pairs)
//   rank cap abs rel v..                          -> kept_rank allowed_error
//   rankfor cap allowed v..                       -> kept_rank_for
//   gram cap abs rel v..                          -> gram_values_decide (0 / 1)
//   route rows cols abs rel frobenius2 SVD        -> hopeless loose jacobi_fits   (SVD: the value of QSV_SVD, "-" = unset)
//   dust L frobenius2                             -> dust_floor2
//   relabel floor2 v..                            -> relabelled | the values | the squared norms afterwards
//   settled rho2 full cap keep abs rel v..        -> settled r compared rho margin allowed r_lo r_hi
//   shares out_rows depth l share_amps            -> split shares
//   options SVD RSVD THREADS ROUNDS TRACE         -> shortcuts jacobi fused_panels svd_threads panel_rounds trace  ("-" = unset)
//   env                                           -> the same six from split_options(), i.e. from this process's environment
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_jacobi.h"
#include "qsv_split_rules.h"

using namespace qsv_split_rules;

static double number(std::istringstream &in) {
    std::string token;
    in >> token;
    return strtod(token.c_str(), nullptr);
}

static std::vector<double> values(std::istringstream &in) {
    size_t n = 0;
    in >> n;
    std::vector<double> v(n);
    for (double &x : v) x = number(in);
    return v;
}

static const char *env_value(const std::string &token) { return token == "-" ? nullptr : token.c_str(); }

static void print_options(const SplitOptions &o) {
    std::printf("%d %d %d %d %d %d\n", o.shortcuts, o.jacobi, o.fused_panels, o.svd_threads, o.panel_rounds, o.trace);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "schedule") {
            int lp = 0;
            in >> lp;
            std::string out;
            for (int step = 0; step < lp - 1; ++step)
                for (int pair = 0; pair < lp / 2; ++pair) {
                    const qsv_jacobi::ColumnPair cp = qsv_jacobi::tournament_pair(lp, step, pair);
                    out += std::to_string(cp.p) + " " + std::to_string(cp.q) + " ";
                }
            std::printf("%s\n", out.c_str());
        } else if (what == "rank") {
            int64_t cap;
            in >> cap;
            const double abs_err = number(in), rel_err = number(in);
            const std::vector<double> sv = values(in);
            std::printf("%" PRIu64 " %a\n", kept_rank(sv, cap, abs_err, rel_err), allowed_error(sv, abs_err, rel_err));
        } else if (what == "rankfor") {
            int64_t cap;
            in >> cap;
            const double allowed = number(in);
            std::printf("%" PRIu64 "\n", kept_rank_for(values(in), cap, allowed));
        } else if (what == "gram") {
            int64_t cap;
            in >> cap;
            const double abs_err = number(in), rel_err = number(in);
            std::printf("%d\n", gram_values_decide(values(in), cap, abs_err, rel_err) ? 1 : 0);
        } else if (what == "route") {
            uint64_t rows, cols;
            in >> rows >> cols;
            const double abs_err = number(in), rel_err = number(in), f2 = number(in);
            std::string svd;
            in >> svd;
            const ExactRoute r = exact_route(rows, cols, abs_err, rel_err, f2, parse_split_options(env_value(svd), nullptr, nullptr, nullptr, nullptr));
            std::printf("%d %d %d\n", r.hopeless, r.loose, r.jacobi_fits);
        } else if (what == "dust") {
            uint64_t L;
            in >> L;
            std::printf("%a\n", dust_floor2(L, number(in)));
        } else if (what == "relabel") {
            const double floor2 = number(in);
            std::vector<double> norm2 = values(in);
            bool relabelled = false;
            const std::vector<double> sv = values_from_norms(norm2, floor2, &relabelled);
            std::printf("%d |", relabelled ? 1 : 0);
            for (double v : sv) std::printf(" %a", v);
            std::printf(" |");
            for (double v : norm2) std::printf(" %a", v);
            std::printf("\n");
        } else if (what == "settled") {
            const double rho2 = number(in);
            uint64_t full;
            int64_t cap, keep;
            in >> full >> cap >> keep;
            const double abs_err = number(in), rel_err = number(in);
            const LowRankVerdict v = low_rank_settled(values(in), rho2, full, cap, keep, abs_err, rel_err);
            std::printf("%d %" PRIu64 " %d %a %a %a %" PRIu64 " %" PRIu64 "\n", v.settled, v.r, v.compared, v.rho, v.margin, v.allowed, v.r_lo,
                        v.r_hi);
        } else if (what == "shares") {
            uint64_t out_rows, depth, share_amps;
            int l;
            in >> out_rows >> depth >> l >> share_amps;
            const SharePlan p = skinny_share_plan(out_rows, depth, l, share_amps);
            std::printf("%u %d\n", p.split, p.shares ? 1 : 0);
        } else if (what == "options") {
            std::string t[5];
            for (std::string &s : t) in >> s;
            print_options(parse_split_options(env_value(t[0]), env_value(t[1]), env_value(t[2]), env_value(t[3]), env_value(t[4])));
        } else if (what == "env") {
            print_options(split_options());
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}

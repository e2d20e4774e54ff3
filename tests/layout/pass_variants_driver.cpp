// TEST INFRASTRUCTURE: what qsv_layout.h::pass_records adds for the pass kernel's body variants, for requests read from
// stdin (tests/test_pass_records_variants_host.py).  Built with AddressSanitizer + UBSan and run on its own.
//
// One request per input line, one answer line per request; doubles are printed as %a.
//   layout                                   -> sizeof(PassGate) then the offsets of form code rc tc tz0 tz1 ctl omask m
//   pass n tile_high count {kind k b0 b1 nctrl cbits.. m[0..32)}..
//        -> status | groups {first count q0..q3 gates}.. | {form code rc tc tz0 tz1 omask m[0..32)}.. | ctl.. |
//           packed omask.. | every_tile | per record: 1 if every byte outside the named fields is zero
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_layout.h"

using namespace qsv_layout;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(PassGate), offsetof(PassGate, form), offsetof(PassGate, code),
                        offsetof(PassGate, rc), offsetof(PassGate, tc), offsetof(PassGate, tz0), offsetof(PassGate, tz1),
                        offsetof(PassGate, ctl), offsetof(PassGate, omask), offsetof(PassGate, m));
        } else if (what == "pass") {
            int n, count;
            unsigned long long tile_high;
            in >> n >> tile_high >> count;
            if (count < 0 || count > qsv_plan::MAX_PASS_GATES) return 2;
            std::vector<Op> ops(count);
            std::vector<const Op *> ptr;
            for (Op &op : ops) {
                in >> op.kind >> op.k >> op.bits[0] >> op.bits[1] >> op.nctrl;
                if (op.nctrl < 0 || op.nctrl > OP_MAX_CTRL) return 2;
                for (int c = 0; c < op.nctrl; ++c) in >> op.cbits[c];
                for (double &x : op.m) in >> x;
                ptr.push_back(&op);
            }
            const PassRecords pr = pass_records(ptr.data(), count, tile_high, 1ull << n);
            std::printf("%d |", static_cast<int>(pr.status));
            if (pr.status == PassRecords::OK) {
                std::printf(" %zu", pr.grp.size());
                for (const PassGroup &g : pr.grp)
                    std::printf(" %d %d %d %d %d %d %llu", g.first, g.count, g.q[0], g.q[1], g.q[2], g.q[3], static_cast<unsigned long long>(g.gates));
                std::printf(" |");
                for (const PassGate &g : pr.rec) {
                    std::printf(" %d %d %u %u %d %d %llu", g.form, g.code, g.rc, g.tc, g.tz0, g.tz1, static_cast<unsigned long long>(g.omask));
                    for (double x : g.m) std::printf(" %a", x);
                }
                std::printf(" |");
                for (const PassGate &g : pr.rec) std::printf(" %d", g.ctl);
                std::printf(" |");
                for (uint64_t o : pr.omask) std::printf(" %llu", static_cast<unsigned long long>(o));
                std::printf(" | %d |", pr.every_tile ? 1 : 0);
                for (const PassGate &g : pr.rec) {      // blank the named fields of a copy: nothing else may be set
                    PassGate z = g;
                    z.form = z.code = z.tz0 = z.tz1 = z.ctl = 0;
                    z.rc = z.tc = 0;
                    z.omask = 0;
                    for (double &x : z.m) x = 0.0;
                    const unsigned char *b = reinterpret_cast<const unsigned char *>(&z);
                    bool clean = true;
                    for (size_t i = 0; i < sizeof(z); ++i) clean = clean && b[i] == 0;
                    std::printf(" %d", clean ? 1 : 0);
                }
            }
        } else {
            return 2;
        }
        if (!in && !in.eof()) return 2;
        std::printf("\n");
    }
    std::fflush(stdout);
    return 0;
}

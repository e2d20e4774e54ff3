// TEST INFRASTRUCTURE: prints the groups qsv_plan.h cuts the gates of a pass into (tests/test_defer_groups_host.py).
//
// Input, repeated until end of file:  count, then `count` target masks (tile indices 0..11 as decimal integers; 0 for a
// gate without targets), in application order.
// Output per pass:  "groups <n>", then per group  "group <first> <count> <reg0> <reg1> <reg2> <reg3>".
#include <cstdio>
#include <vector>

#include "qsv_plan.h"

int main() {
    int count = 0;
    while (std::scanf("%d", &count) == 1) {
        if (count < 0) return 2;
        std::vector<uint32_t> need(count);
        for (auto &m : need) {
            unsigned v = 0;
            if (std::scanf("%u", &v) != 1) return 2;
            m = v;
        }
        const std::vector<qsv_plan::Group> groups = qsv_plan::cut_groups(need);
        std::printf("groups %zu\n", groups.size());
        for (const auto &g : groups)
            std::printf("group %d %d %d %d %d %d\n", g.first, g.count, g.reg[0], g.reg[1], g.reg[2], g.reg[3]);
        std::fflush(stdout);
    }
    return 0;
}

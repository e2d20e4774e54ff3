// TEST INFRASTRUCTURE: prints the plan qsv_plan.h makes for gate lists read from stdin (tests/test_defer_plan_host.py).
//
// Input, repeated until end of file:  n window count, then `count` lines  need ctrl exact cost  (need, ctrl: register bit
// masks as decimal integers; exact: 0 / 1; cost: per-gate launch cost in full passes).
// Output per gate list:  "plan <passes>", then per pass  "pass <fused> <tile mask> <gates>"  followed by one line
// "gate <queue index> <control mask inside the tile, tile indices> <control mask outside the tile, register bits>" per
// gate, in application order.
#include <cstdio>
#include <vector>

#include "qsv_plan.h"

int main() {
    int n = 0, count = 0;
    unsigned long long window = 0;
    while (std::scanf("%d %llu %d", &n, &window, &count) == 3) {
        std::vector<qsv_plan::Gate> q(count);
        for (auto &g : q) {
            unsigned long long need = 0, ctrl = 0;
            int exact = 0;
            float cost = 1.0f;
            if (std::scanf("%llu %llu %d %f", &need, &ctrl, &exact, &cost) != 4) return 2;
            g.need = need;
            g.ctrl = ctrl;
            g.exact = exact != 0;
            g.cost = cost;
        }
        const std::vector<qsv_plan::Pass> plan = qsv_plan::plan_stream(q, n, window);
        std::printf("plan %zu\n", plan.size());
        for (const auto &p : plan) {
            std::printf("pass %d %llu %zu\n", p.fused ? 1 : 0, static_cast<unsigned long long>(p.tile), p.gates.size());
            for (int i : p.gates) {
                const qsv_plan::ControlMasks cm = qsv_plan::control_masks(q[i].ctrl, p.tile);
                std::printf("gate %d %u %llu\n", i, cm.inside, static_cast<unsigned long long>(cm.outside));
            }
        }
        std::fflush(stdout);
    }
    return 0;
}

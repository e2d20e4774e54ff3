// TEST INFRASTRUCTURE: answers questions about qsv_channel_layout.h on the host (tests/test_channel_layout_host.py).
// One request per input line, one answer line each:
//   plan n k b0 b1 streaming cap
//     -> W kh kl | pos.. | hoff[0..3] | lbit.. | lxor[0..3] | ghi[0..3] | glo[0..3] | rdm_grid apply_grid |
//        checked cover_min cover_max bad_group bad_partner bad_range
//      where the last part walks the launch shape as the kernels do: every work item w, every high combination h owns
//      amplitude item_base(w) + hoff[h]; its group index must be that of the amplitude's own target bits, and the partner
//      lane of low combination dl must own the amplitude that differs in exactly those lane bits.  Registers up to 2^16
//      amplitudes are walked whole (cover_min = cover_max = 1 means every amplitude exactly once); larger ones at their
//      ends and at 4096 scattered items, where cover_* report the bijection test on the bit positions instead.
//   slots D -> rdm_entries | rdm_pair_slot(r, c) for r < c in row-major order
//   pick u w0 w1 ... -> branch total
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_channel_layout.h"

using namespace qsv_channel_layout;

static int group_of(uint64_t idx, int k, const int *bits) {
    int g = 0;
    for (int j = 0; j < k; ++j) g |= static_cast<int>((idx >> bits[j]) & 1ull) << (k - 1 - j);
    return g;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "plan") {
            int n, k, bits[2], streaming, cap;
            in >> n >> k >> bits[0] >> bits[1] >> streaming >> cap;
            const uint64_t amps = 1ull << n;
            const ChannelPlan p = channel_plan(n, amps, k, bits, streaming != 0);
            const ChannelArgs &g = p.g;
            std::printf("%" PRIu64 " %d %d |", g.W, p.kh, p.kl);
            for (int i = 0; i < p.kh; ++i) std::printf(" %u", g.pos[i]);
            std::printf(" |");
            for (int c = 0; c < 4; ++c) std::printf(" %" PRIu64, g.hoff[c]);
            std::printf(" |");
            for (int i = 0; i < p.kl; ++i) std::printf(" %d", g.lbit[i]);
            std::printf(" |");
            for (int c = 0; c < 4; ++c) std::printf(" %d", g.lxor[c]);
            std::printf(" |");
            for (int c = 0; c < 4; ++c) std::printf(" %d", g.ghi[c]);
            std::printf(" |");
            for (int c = 0; c < 4; ++c) std::printf(" %d", g.glo[c]);
            std::printf(" | %d %d |", rdm_grid(g.W, cap), apply_grid(g.W, cap));
            const int NH = 1 << p.kh, NL = 1 << p.kl;
            const bool whole = n <= 16;
            std::vector<uint8_t> seen(whole ? amps : 0, 0);
            uint64_t bad_group = 0, bad_partner = 0, bad_range = 0, checked = 0;
            auto visit = [&](uint64_t w) {
                const uint64_t base = item_base(g, w);
                const int l_own = lane_combination(g, static_cast<uint32_t>(w & 63));
                for (int h = 0; h < NH; ++h) {
                    const uint64_t idx = base + g.hoff[h];
                    ++checked;
                    if (idx >= amps) {
                        ++bad_range;
                        continue;
                    }
                    if (whole && seen[idx] < 255) ++seen[idx];
                    if (group_of(idx, k, bits) != (g.ghi[h] | g.glo[l_own])) ++bad_group;
                    for (int dl = 1; dl < NL; ++dl) {
                        const uint64_t w2 = w ^ static_cast<uint64_t>(g.lxor[dl]);
                        const uint64_t idx2 = item_base(g, w2) + g.hoff[h];
                        // the partner sits in the same 64-amplitude segment, differs in the lane bits of dl only, and owns
                        // the group index the kernels assume for it
                        if (w2 >= g.W || (w2 >> 6) != (w >> 6) || idx2 != (idx ^ static_cast<uint64_t>(g.lxor[dl])) ||
                            group_of(idx2, k, bits) != (g.ghi[h] | g.glo[l_own ^ dl]))
                            ++bad_partner;
                    }
                }
            };
            int cover_min = 255, cover_max = 0;
            if (whole) {
                for (uint64_t w = 0; w < g.W; ++w) visit(w);
                for (uint64_t i = 0; i < amps; ++i) {
                    cover_min = std::min<int>(cover_min, seen[i]);
                    cover_max = std::max<int>(cover_max, seen[i]);
                }
            } else {
                uint64_t state = 0x9E3779B97F4A7C15ull ^ (static_cast<uint64_t>(n) << 32) ^ static_cast<uint64_t>(bits[0] * 64 + bits[1]);
                for (uint64_t w : {uint64_t(0), uint64_t(1), uint64_t(63), uint64_t(64), g.W / 2, g.W - 64, g.W - 1}) visit(w);
                for (int s = 0; s < 4096; ++s) {
                    state = state * 6364136223846793005ull + 1442695040888963407ull;
                    visit((state >> 11) % g.W);
                }
                // (w, h) -> index is a bijection onto [0, amps) iff the inserted positions are distinct bits of the register in
                // ascending order, hoff[h] is exactly the OR of the positions h selects, and W 2^kh = amps
                bool ok = (g.W << p.kh) == amps;
                for (int i = 0; i < p.kh; ++i) ok = ok && g.pos[i] < static_cast<uint32_t>(n) && (i == 0 || g.pos[i] > g.pos[i - 1]);
                for (int h = 0; h < NH; ++h) {
                    uint64_t want = 0;
                    for (int i = 0; i < p.kh; ++i)
                        if ((h >> i) & 1) want |= 1ull << g.pos[i];
                    ok = ok && g.hoff[h] == want;
                }
                cover_min = cover_max = ok ? 1 : 0;
            }
            std::printf(" %" PRIu64 " %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", checked, cover_min, cover_max, bad_group, bad_partner, bad_range);
        } else if (what == "slots") {
            int D;
            in >> D;
            std::printf("%d |", rdm_entries(D));
            for (int r = 0; r < D; ++r)
                for (int c = r + 1; c < D; ++c) std::printf(" %d", rdm_pair_slot(D, r, c));
            std::printf("\n");
        } else if (what == "pick") {
            double u, x;
            std::vector<double> w;
            in >> u;
            while (in >> x) w.push_back(x);
            double total = -1.0;
            const int j = pick_branch(w.data(), static_cast<int>(w.size()), u, &total);
            std::printf("%d %.17g\n", j, total);
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}

// TEST INFRASTRUCTURE: answers questions about qsv_ensemble_layout.h on the host (tests/test_ensemble_layout_host.py).
// One request per input line, one answer line each:
//   case n b k b0 b1 lanes cap
//     -> kh kl item_bits | read: part_bits share_bits units grid | update: part_bits share_bits units grid |
//        read: checked cover_min cover_max bad_owner bad_mix bad_wave | update: the same |
//        slots partials matrix draws log doubles
//   where the two walks follow the kernels: thread tid of unit u works on member ens_thread().member and on the items
//   first_item, first_item + stride, ... of that member, and owns the amplitudes member 2^n + item_base(item) + hoff[h].
//   Registers of at most 2^12 amplitudes are walked whole (cover_min = cover_max = 1: every amplitude exactly once); larger
//   ones at scattered amplitudes whose owner (ens_owner) must be the thread that ens_thread sends there (cover_* are 1 then).
//   bad_owner: ens_owner and ens_thread disagree.  bad_mix: lanes of one summed segment, or waves added together, that belong
//   to different members.  bad_wave: in the lane form, a wave whose lanes are not 64 consecutive items of one member.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_ensemble_layout.h"

using namespace qsv_channel_layout;
using namespace qsv_ensemble_layout;

struct Walk {
    uint64_t checked = 0, cover_min = 1, cover_max = 1, bad_owner = 0, bad_mix = 0, bad_wave = 0;
};

static void check_unit(const EnsArgs &e, const ChannelPlan &p, uint64_t unit, Walk &out) {
    EnsThread t[CH_BLOCK];
    for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) t[tid] = ens_thread(e, unit, tid);
    const int segment = ens_segment_lanes(e), waves = ens_waves_per_member(e);
    for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
        if (t[tid].member != t[tid & ~static_cast<uint32_t>(segment - 1)].member) ++out.bad_mix;       // the butterfly's run
        const uint32_t wave = tid >> 6, first_wave = wave / waves * waves;
        if (e.item_bits >= 6 && t[tid].member != t[first_wave * 64].member) ++out.bad_mix;              // the waves added in LDS
        if (e.item_bits >= 6 && t[tid].member != (((unit >> e.part_bits) << e.share_bits) + first_wave / waves)) ++out.bad_mix;
        if (p.kl > 0) {
            const uint32_t lane0 = tid & ~63u;
            if (t[tid].member != t[lane0].member || t[tid].first_item != t[lane0].first_item + (tid & 63u) || (t[lane0].first_item & 63u)) ++out.bad_wave;
            if ((t[tid].stride & 63u) || e.item_bits < 6) ++out.bad_wave;
        }
    }
}

static Walk walk(const EnsArgs &e, const ChannelPlan &p, int n) {
    Walk out;
    const uint64_t amps = e.members << n, items = 1ull << e.item_bits;
    const int NH = 1 << p.kh;
    if (amps <= (1ull << 12)) {
        std::vector<uint32_t> seen(amps, 0);
        for (uint64_t unit = 0; unit < e.units; ++unit) {
            check_unit(e, p, unit, out);
            for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
                const EnsThread t = ens_thread(e, unit, tid);
                if (t.member >= e.members) continue;
                for (uint64_t w = t.first_item; w < items; w += t.stride) {
                    const EnsOwner o = ens_owner(e, t.member, w);
                    if (o.unit != unit || o.tid != tid || o.part != t.part) ++out.bad_owner;
                    for (int h = 0; h < NH; ++h) {
                        const uint64_t idx = (t.member << n) + item_base(p.g, w) + p.g.hoff[h];
                        if (idx >= amps) { ++out.bad_owner; continue; }
                        ++seen[idx];
                        if (ens_member_of(n, idx) != t.member || ens_item_of(p.g, ens_local_of(n, idx)) != w) ++out.bad_owner;
                        ++out.checked;
                    }
                }
            }
        }
        out.cover_min = out.cover_max = seen[0];
        for (uint32_t c : seen) {
            out.cover_min = std::min<uint64_t>(out.cover_min, c);
            out.cover_max = std::max<uint64_t>(out.cover_max, c);
        }
        return out;
    }
    // scattered amplitudes and both ends; the units they fall in
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int s = 0; s < 16; ++s) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t idx = s == 0 ? 0 : s == 1 ? amps - 1 : x % amps;
        const uint64_t member = ens_member_of(n, idx), item = ens_item_of(p.g, ens_local_of(n, idx));
        const EnsOwner o = ens_owner(e, member, item);
        if (o.unit >= e.units || o.tid >= CH_BLOCK) { ++out.bad_owner; continue; }
        const EnsThread t = ens_thread(e, o.unit, o.tid);
        const bool visits = t.member == member && member < e.members && item >= t.first_item && (item - t.first_item) % t.stride == 0 && item < items;
        bool owns = false;
        for (int h = 0; h < NH; ++h) owns = owns || (member << n) + item_base(p.g, item) + p.g.hoff[h] == idx;
        if (!visits || !owns || t.part != o.part) ++out.bad_owner;
        if (s < 3) check_unit(e, p, o.unit, out);     // both ends and one in between
        ++out.checked;
    }
    return out;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what != "case") {
            std::printf("?\n");
            continue;
        }
        int n, b, k, bits[2], lanes, cap;
        in >> n >> b >> k >> bits[0] >> bits[1] >> lanes >> cap;
        const uint64_t members = 1ull << b;
        const bool use_lanes = ens_lanes(n, lanes != 0);
        const ChannelPlan p = ens_channel_plan(n, k, bits, use_lanes);
        const int item_bits = n - p.kh;
        const EnsArgs read = ens_args(n, members, item_bits, part_bits(item_bits, cap));
        const EnsArgs update = ens_args(n, members, item_bits, apply_part_bits(item_bits, cap));
        std::printf("%d %d %d %" PRIu64 " |", p.kh, p.kl, item_bits, p.g.W);
        for (const EnsArgs *e : {&read, &update}) std::printf(" %d %d %" PRIu64 " %d |", e->part_bits, e->share_bits, e->units, ens_grid(*e, cap));
        for (const EnsArgs *e : {&read, &update}) {
            const Walk w = walk(*e, p, n);
            std::printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " |", w.checked, w.cover_min, w.cover_max, w.bad_owner,
                        w.bad_mix, w.bad_wave);
        }
        const EnsWorkspace ws = ens_workspace(n, members);
        std::printf(" %d %zu %zu %zu %zu %zu\n", ws.slots, ws.partials, ws.matrix, ws.draws, ws.log, ws.doubles);
    }
    return 0;
}

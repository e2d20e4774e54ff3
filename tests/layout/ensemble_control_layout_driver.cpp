// TEST INFRASTRUCTURE: answers questions about qsv_ensemble_control_layout.h on the host
// (tests/test_ensemble_control_layout_host.py).  One request per input line, one answer line each:
//   case n b k b0 b1 lanes cap
//     -> kh kl item_bits | part_bits share_bits units grid uniform lanes_safe chunk_bits |
//        checked takers cover_min cover_max touched bad_owner bad_partner bad_unit bad_batch
//   The walk follows k_ens_apply_conditional: thread tid of unit u tests the word of cond_thread_member(e, u, tid); if the word
//   satisfies the masks it works on the items first_item, first_item + stride, ... of ens_thread().member and owns the
//   amplitudes member 2^n + item_base(item) + hoff[h].  The words are a fixed hash of the member index with all_of = 1 and
//   none_of = 2, so about a quarter of the members take the gate; member 0 is made a taker and the last member a non-taker
//   where there are two or more.
//   Registers of at most 2^12 amplitudes are walked whole: cover_min / cover_max are the fewest and the most owners of an
//   amplitude of a TAKING member (1 and 1), touched the amplitudes of other members that any thread owns (0).  Larger ones at
//   scattered amplitudes, whose owner (ens_owner) must be the thread that ens_thread sends there and must test that member's
//   word (cover_* are 1 then, touched 0).
//   bad_owner: ens_owner and ens_thread disagree, or an owned amplitude lies in another member than the one tested.
//   bad_partner: a lane whose shfl_xor partner (any low combination of the plan) tests another member's word.
//   bad_unit: a unit that lies in one member whose threads do not all work on cond_unit_member(unit), or a member index
//   beyond the ensemble there.
//   bad_batch: a unit that the chunked walk of a workgroup's units (workgroup g of cond_grid takes the chunks g, g + grid, ...;
//   lane l < 2^chunk_bits of a chunk looks at unit cond_batch_unit(chunk, l, chunk_bits)) does not visit exactly once, or that
//   cond_visit_of places elsewhere.  Up to 2^12 units are walked whole, more at 16 scattered units and with the chunks counted.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_ensemble_control_layout.h"

using namespace qsv_channel_layout;
using namespace qsv_ensemble_layout;
using namespace qsv_ensemble_control_layout;

constexpr uint64_t ALL_OF = 1, NONE_OF = 2;

static uint64_t word_of(uint64_t member, uint64_t members) {
    if (member == 0) return 1;
    if (member == members - 1) return 3;
    uint64_t x = (member + 1) * 0x9e3779b97f4a7c15ull;
    x ^= x >> 29;
    return x;
}

struct Walk {
    uint64_t checked = 0, takers = 0, cover_min = 1, cover_max = 1, touched = 0, bad_owner = 0, bad_partner = 0, bad_unit = 0;
};

static void check_unit(const EnsArgs &e, const ChannelPlan &p, uint64_t unit, Walk &out) {
    for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
        const uint64_t tested = cond_thread_member(e, unit, tid);
        if (cond_unit_uniform(e)) {
            if (ens_thread(e, unit, tid).member != cond_unit_member(e, unit) || tested != cond_unit_member(e, unit) || tested >= e.members) ++out.bad_unit;
        } else if (tested != ens_thread(e, unit, tid).member) {
            ++out.bad_unit;
        }
        for (int l = 0; l < (1 << p.kl); ++l)
            if (cond_partner_member(e, p.g, unit, tid, l) != tested) ++out.bad_partner;
    }
}

static uint64_t batch_walk(const EnsArgs &e, int chunk_bits, uint64_t grid) {
    uint64_t bad = 0;
    const uint64_t chunks = cond_chunks(e);
    if ((chunks << chunk_bits) < e.units || ((chunks - 1) << chunk_bits) >= e.units) ++bad;     // the chunks cover the units, none is empty
    auto placed = [&](uint64_t unit) {
        const CondVisit v = cond_visit_of(unit, chunk_bits, grid);
        return v.block < grid && v.lane < (1u << chunk_bits) && v.chunk < chunks && (v.chunk - v.block) % grid == 0 &&
               cond_batch_unit(v.chunk, v.lane, chunk_bits) == unit;
    };
    if (e.units <= 4096) {
        std::vector<uint32_t> visits(e.units, 0);
        for (uint64_t block = 0; block < grid; ++block)
            for (uint64_t chunk = block; chunk < chunks; chunk += grid)
                for (uint32_t lane = 0; lane < (1u << chunk_bits); ++lane) {
                    const uint64_t unit = cond_batch_unit(chunk, lane, chunk_bits);
                    if (unit < e.units) ++visits[unit];
                }
        for (uint64_t unit = 0; unit < e.units; ++unit)
            if (visits[unit] != 1 || !placed(unit)) ++bad;
        return bad;
    }
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (int s = 0; s < 16; ++s) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        if (!placed(s == 0 ? 0 : s == 1 ? e.units - 1 : x % e.units)) ++bad;
    }
    return bad;
}

static Walk walk(const EnsArgs &e, const ChannelPlan &p, int n) {
    Walk out;
    const uint64_t amps = e.members << n, items = 1ull << e.item_bits;
    const int NH = 1 << p.kh;
    for (uint64_t m = 0; m < e.members; ++m) out.takers += takes(word_of(m, e.members), ALL_OF, NONE_OF) ? 1 : 0;
    if (amps <= (1ull << 12)) {
        std::vector<uint32_t> seen(amps, 0);
        for (uint64_t unit = 0; unit < e.units; ++unit) {
            check_unit(e, p, unit, out);
            for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
                const EnsThread t = ens_thread(e, unit, tid);
                if (t.member >= e.members) continue;
                const uint64_t tested = cond_thread_member(e, unit, tid);
                if (!takes(word_of(tested, e.members), ALL_OF, NONE_OF)) continue;
                for (uint64_t w = t.first_item; w < items; w += t.stride) {
                    const EnsOwner o = ens_owner(e, t.member, w);
                    if (o.unit != unit || o.tid != tid || o.part != t.part) ++out.bad_owner;
                    for (int h = 0; h < NH; ++h) {
                        const uint64_t idx = (t.member << n) + item_base(p.g, w) + p.g.hoff[h];
                        if (idx >= amps) { ++out.bad_owner; continue; }
                        ++seen[idx];
                        if (ens_member_of(n, idx) != tested) ++out.bad_owner;
                        ++out.checked;
                    }
                }
            }
        }
        bool first = true;
        for (uint64_t idx = 0; idx < amps; ++idx) {
            if (takes(word_of(ens_member_of(n, idx), e.members), ALL_OF, NONE_OF)) {
                if (first) out.cover_min = out.cover_max = seen[idx];
                first = false;
                out.cover_min = std::min<uint64_t>(out.cover_min, seen[idx]);
                out.cover_max = std::max<uint64_t>(out.cover_max, seen[idx]);
            } else {
                out.touched += seen[idx];
            }
        }
        return out;
    }
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
        if (!visits || !owns || t.part != o.part || cond_thread_member(e, o.unit, o.tid) != member) ++out.bad_owner;
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
        const ChannelPlan p = ens_channel_plan(n, k, bits, ens_lanes(n, lanes != 0));
        const int item_bits = n - p.kh;
        const EnsArgs e = ens_args(n, members, item_bits, apply_part_bits(item_bits, cap));
        const Walk w = walk(e, p, n);
        const int grid = cond_grid(e, cap);
        const int chunk_bits = cond_unit_uniform(e) ? cond_chunk_bits(e.units) : 0;
        std::printf("%d %d %d | %d %d %" PRIu64 " %d %d %d %d | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
                    p.kh, p.kl, item_bits, e.part_bits, e.share_bits, e.units, grid, cond_unit_uniform(e) ? 1 : 0, cond_lanes_safe(e, p.kl) ? 1 : 0, chunk_bits,
                    w.checked, w.takers, w.cover_min, w.cover_max, w.touched, w.bad_owner, w.bad_partner, w.bad_unit,
                    grid >= 1 ? batch_walk(e, chunk_bits, static_cast<uint64_t>(grid)) : 1);
    }
    return 0;
}

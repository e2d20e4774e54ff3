// TEST INFRASTRUCTURE: answers questions about qsv_sweep_layout.h on the host (tests/test_sweep_layout_host.py).  One request
// per input line, one answer line each:
//   case n b pivot cap      (pivot = -1: the diagonal form)
//     -> item_bits part_bits share_bits units grid wave unit | checked cover_min cover_max bad_owner bad_member bad_table bad_uniform
//   The walk follows k_ens_pauli_rotate_group: thread tid of unit u (ens_thread) works on the items first_item,
//   first_item + stride, ... of its member and owns amplitude w of the member (diagonal) or the pair {i, i ^ xmask} with
//   i = insert_zero(w, pivot).  The xmask has the pivot as its highest bit and every second bit below it.
//   Registers of at most 2^12 amplitudes are walked whole: cover_min / cover_max are the fewest and the most owners of an
//   amplitude (1 and 1).  Larger ones at scattered amplitudes, whose owner (item_of, ens_owner) must be the thread that
//   ens_thread sends there (cover_* are 1 then).
//   bad_owner: ens_owner and ens_thread disagree, or an owned index lies outside the register.
//   bad_member: an amplitude of a pair that lies in another member than its owner's.
//   bad_table: a table offset of (member, slot t < 8, cos / sin) outside the allocation, or one of a slot t < count outside the
//   [members][n_terms][2] part or not at [member][first + t], for passes of 1 .. 8 terms that start anywhere in a list of 19
//   terms, at the first and the last member.
//   bad_uniform: a wave (64 consecutive threads of a unit) whose threads work on more than one member although
//   wave_in_one_member says one, or a unit whose threads do although unit_in_one_member says one.
//   table n_terms members -> doubles
//   expect n b cap -> item_bits part_bits share_bits units grid values doubles      (the read pass of k_ens_diag_expect)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_sweep_layout.h"

using namespace qsv_ensemble_layout;
using namespace qsv_sweep_layout;

struct Walk {
    uint64_t checked = 0, cover_min = 1, cover_max = 1, bad_owner = 0, bad_member = 0, bad_table = 0, bad_uniform = 0;
};

static uint64_t xmask_of(int pivot) {
    uint64_t x = 0;
    for (int bit = pivot; bit >= 0; bit -= 2) x |= 1ull << bit;
    return x;
}

static void check_unit(const EnsArgs &e, uint64_t unit, Walk &out) {
    for (uint32_t wave = 0; wave < CH_BLOCK / 64; ++wave) {
        const uint64_t first = ens_thread(e, unit, wave * 64).member;
        for (uint32_t lane = 1; lane < 64; ++lane)
            if (wave_in_one_member(e) && ens_thread(e, unit, wave * 64 + lane).member != first) ++out.bad_uniform;
    }
    for (uint32_t tid = 1; tid < CH_BLOCK; ++tid)
        if (unit_in_one_member(e) && ens_thread(e, unit, tid).member != ens_thread(e, unit, 0).member) ++out.bad_uniform;
}

static uint64_t table_walk(uint64_t members) {
    uint64_t bad = 0;
    const int n_terms = 19;
    const size_t doubles = table_doubles(members, n_terms);
    for (int first = 0; first < n_terms; ++first)
        for (int count = 1; count <= 8 && first + count <= n_terms; ++count) {
            const SweepArgs s = sweep_args(n_terms, first, count);
            for (uint64_t member : {uint64_t(0), members - 1})
                for (int t = 0; t < SWEEP_MAX_SLOTS; ++t)
                    for (int part = 0; part < 2; ++part) {
                        const size_t at = table_offset(s, member, t, part);
                        // every slot the kernel may fetch lies inside the allocation; a slot it uses lies inside the
                        // [members][n_terms][2] part, where [member][first + t][part] is
                        if (at >= doubles) ++bad;
                        if (t < count && (at >= doubles - TABLE_PAD || at != (static_cast<size_t>(member) * n_terms + first + t) * 2 + part)) ++bad;
                    }
        }
    return bad;
}

static Walk walk(const EnsArgs &e, int n, bool diag, int pivot) {
    Walk out;
    const uint64_t amps = e.members << n, items = 1ull << e.item_bits, xmask = diag ? 0 : xmask_of(pivot);
    auto owned = [&](uint64_t member, uint64_t w, uint64_t idx[2]) {
        const uint64_t i = diag ? w : insert_zero(w, pivot);
        idx[0] = (member << n) + i;
        idx[1] = (member << n) + (i ^ xmask);
        for (int h = 0; h < (diag ? 1 : 2); ++h)
            if (idx[h] >= amps || ens_member_of(n, idx[h]) != member) ++out.bad_member;
    };
    if (amps <= (1ull << 12)) {
        std::vector<uint32_t> seen(amps, 0);
        for (uint64_t unit = 0; unit < e.units; ++unit) {
            check_unit(e, unit, out);
            for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
                const EnsThread t = ens_thread(e, unit, tid);
                if (t.member >= e.members) continue;
                for (uint64_t w = t.first_item; w < items; w += t.stride) {
                    const EnsOwner o = ens_owner(e, t.member, w);
                    if (o.unit != unit || o.tid != tid || o.part != t.part) ++out.bad_owner;
                    uint64_t idx[2];
                    owned(t.member, w, idx);
                    for (int h = 0; h < (diag ? 1 : 2); ++h) {
                        if (idx[h] >= amps) { ++out.bad_owner; continue; }
                        ++seen[idx[h]];
                        ++out.checked;
                    }
                }
            }
        }
        out.cover_min = out.cover_max = seen[0];
        for (uint64_t idx = 0; idx < amps; ++idx) {
            out.cover_min = std::min<uint64_t>(out.cover_min, seen[idx]);
            out.cover_max = std::max<uint64_t>(out.cover_max, seen[idx]);
        }
        return out;
    }
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int s = 0; s < 16; ++s) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t idx = s == 0 ? 0 : s == 1 ? amps - 1 : x % amps;
        const uint64_t member = ens_member_of(n, idx), local = ens_local_of(n, idx);
        // the pair's element with a clear pivot bit is the one the item is numbered by
        const uint64_t base = (!diag && ((local >> pivot) & 1)) ? local ^ xmask : local;
        const uint64_t item = item_of(base, diag, pivot);
        const EnsOwner o = ens_owner(e, member, item);
        if (o.unit >= e.units || o.tid >= CH_BLOCK || item >= items) { ++out.bad_owner; continue; }
        const EnsThread t = ens_thread(e, o.unit, o.tid);
        const bool visits = t.member == member && item >= t.first_item && (item - t.first_item) % t.stride == 0 && t.part == o.part;
        uint64_t got[2];
        owned(member, item, got);
        if (!visits || (got[0] != idx && (diag || got[1] != idx))) ++out.bad_owner;
        if (s < 3) check_unit(e, o.unit, out);     // both ends and one in between
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
        if (what == "table") {
            int n_terms;
            uint64_t members;
            in >> n_terms >> members;
            std::printf("%zu\n", table_doubles(members, n_terms));
            continue;
        }
        if (what == "expect") {
            int n, b, cap;
            in >> n >> b >> cap;
            const EnsArgs e = expect_args(n, 1ull << b, cap);
            std::printf("%d %d %d %" PRIu64 " %d %zu %zu\n", e.item_bits, e.part_bits, e.share_bits, e.units, ens_grid(e, cap), expect_values(e.members),
                        expect_doubles(e));
            continue;
        }
        if (what != "case") {
            std::printf("?\n");
            continue;
        }
        int n, b, pivot, cap;
        in >> n >> b >> pivot >> cap;
        const bool diag = pivot < 0;
        const uint64_t members = 1ull << b;
        const EnsArgs e = rotate_args(n, members, diag, cap);
        Walk w = walk(e, n, diag, pivot);
        w.bad_table = table_walk(members);
        std::printf("%d %d %d %" PRIu64 " %d %d %d | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", e.item_bits,
                    e.part_bits, e.share_bits, e.units, ens_grid(e, cap), wave_in_one_member(e) ? 1 : 0, unit_in_one_member(e) ? 1 : 0, w.checked,
                    w.cover_min, w.cover_max, w.bad_owner, w.bad_member, w.bad_table, w.bad_uniform);
    }
    return 0;
}

// TEST INFRASTRUCTURE: answers questions about the adjoint-walk part of qsv_sweep_layout.h on the host
// (tests/test_ensemble_adjoint_layout_host.py).  One request per input line, one answer line each:
//   case n b pivot cap      (pivot = -1: the diagonal form)
//     -> item_bits part_bits share_bits units grid wave | checked cover_min cover_max bad_owner bad_member bad_table bad_partial bad_fit
//   The walk follows k_ens_pauli_adjoint_group: thread tid of unit u (ens_thread) works on the items first_item,
//   first_item + stride, ... of its member and owns, in BOTH registers, amplitude w of the member (diagonal) or the pair
//   {i, i ^ xmask} with i = insert_zero(w, pivot).  The xmask has the pivot as its highest bit and every second bit below it.
//   Registers of at most 2^12 amplitudes are walked whole: cover_min / cover_max are the fewest and the most owners of an
//   amplitude (1 and 1).  Larger ones at scattered amplitudes, whose owner (item_of, ens_owner) must be the thread that
//   ens_thread sends there, and at all threads of the first and the last unit.
//   bad_owner: ens_owner and ens_thread disagree, or an owned index lies outside the register.
//   bad_member: an amplitude of a pair that lies in another member than its owner's.
//   bad_table: for EVERY thread of a visited unit, live or not, the member whose row it fetches (adjoint_fetch_member) is not a
//   member, or a table offset of (that member, slot t < 8, cos / sin) lies outside the allocation, or one of a slot t < count
//   is not at [member][first + count - 1 - t]; passes of 1, 5 and 8 terms at the start and the end of a list of 19 terms.
//   bad_partial: a partial slot (member, part, slot, re / im) of a live thread, for widths 1, 2, 4 and 8, outside the
//   workspace's [members][P_max][16] partials, or two (member, part) that share a slot.
//   bad_fit: adjoint_fits_workspace says no for a width, or the results or the table leave the scratch buffer.
//   pair n b cap -> item_bits part_bits share_bits units grid | bad_partial bad_values      (k_ens_inner, k_ens_diag_phase_adjoint)
//   gpusizes -> the sizes of tests/test_gpu_ensemble_adjoint.py with parts >= 2 and grid < units, as n:b:cap:form
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_sweep_layout.h"

using namespace qsv_ensemble_layout;
using namespace qsv_sweep_layout;

struct Walk {
    uint64_t checked = 0, cover_min = 1, cover_max = 1, bad_owner = 0, bad_member = 0, bad_table = 0, bad_partial = 0, bad_fit = 0;
};

static uint64_t xmask_of(int pivot) {
    uint64_t x = 0;
    for (int bit = pivot; bit >= 0; bit -= 2) x |= 1ull << bit;
    return x;
}

// what every thread of a unit does before and after its item loop: the table fetch and the partial slots
static void check_unit(const EnsArgs &e, uint64_t unit, Walk &out) {
    const int n_terms = 19;
    const size_t table = table_doubles(e.members, n_terms);
    const EnsWorkspace ws = ens_workspace(e.n, e.members);
    const size_t room = ws.matrix - ws.partials;
    for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
        const EnsThread t = ens_thread(e, unit, tid);
        const uint64_t fetch = adjoint_fetch_member(e, t.member);
        if (fetch >= e.members) ++out.bad_table;
        if (t.member < e.members && fetch != t.member) ++out.bad_table;
        for (int first : {0, n_terms - 8})
            for (int count : {1, 5, 8}) {
                const SweepArgs s = sweep_args(n_terms, first, count);
                for (int slot = 0; slot < SWEEP_MAX_SLOTS; ++slot)
                    for (int part = 0; part < 2; ++part) {
                        const size_t at = adjoint_table_offset(s, fetch, slot, part);
                        if (at >= table) ++out.bad_table;
                        if (slot < count && at != (static_cast<size_t>(fetch) * n_terms + first + count - 1 - slot) * 2 + part) ++out.bad_table;
                    }
            }
        if (t.member >= e.members) continue;
        for (int width : {1, 2, 4, 8})
            for (int slot = 0; slot < width; ++slot)
                for (int c = 0; c < 2; ++c) {
                    const size_t at = adjoint_partial_offset(e, t.member, t.part, width, slot, c);
                    if (at >= room || at >= adjoint_partial_doubles(e, width)) ++out.bad_partial;
                    // (member, part) -> slot is one to one: the block of 2 width doubles is where the formula says and nowhere else
                    if (at / (2 * width) != (t.member << e.part_bits) + t.part || t.part >= (1ull << e.part_bits)) ++out.bad_partial;
                }
    }
}

static Walk walk(const EnsArgs &e, int n, bool diag, int pivot) {
    Walk out;
    const uint64_t amps = e.members << n, items = 1ull << e.item_bits, xmask = diag ? 0 : xmask_of(pivot);
    for (int width : {1, 2, 4, 8})
        if (!adjoint_fits_workspace(e, width)) ++out.bad_fit;
    if (adjoint_scratch_doubles(e.members, 19) != table_doubles(e.members, 19) + e.members * 19 * 2) ++out.bad_fit;
    if (adjoint_results_offset(e.members, 19) < e.members * 19 * 2 + TABLE_PAD) ++out.bad_fit;
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
    check_unit(e, 0, out);
    check_unit(e, e.units - 1, out);
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
        if (s == 2) check_unit(e, o.unit, out);     // one in between
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
        if (what == "pair") {
            int n, b, cap;
            in >> n >> b >> cap;
            const uint64_t members = 1ull << b;
            const EnsArgs e = pair_args(n, members, cap);
            const EnsWorkspace ws = ens_workspace(n, members);
            uint64_t bad_partial = 0, bad_values = 0;
            std::set<uint64_t> units = {0, e.units / 2, e.units - 1};
            for (uint64_t unit : units)
                for (uint32_t tid = 0; tid < CH_BLOCK; ++tid) {
                    const EnsThread t = ens_thread(e, unit, tid);
                    if (t.member >= members) continue;
                    const size_t at = ((static_cast<size_t>(t.member) << e.part_bits) + t.part) * SWEEP_PAIR_SLOTS + 1;
                    if (at >= ws.matrix - ws.partials || at >= pair_partial_doubles(e)) ++bad_partial;
                }
            if (pair_values(members) > ws.draws - ws.matrix) ++bad_values;
            std::printf("%d %d %d %" PRIu64 " %d | %" PRIu64 " %" PRIu64 "\n", e.item_bits, e.part_bits, e.share_bits, e.units, ens_grid(e, cap), bad_partial,
                        bad_values);
            continue;
        }
        if (what == "gpusizes") {
            std::string out;
            for (int n : {1, 2, 3, 7, 8, 9, 13, 14, 15})
                for (int b : {0, 1, 3, 6})
                    for (int cap : {0, 2})
                        for (int diag = 0; diag < 2; ++diag) {
                            if (n + b > 18 || (cap && n < 13)) continue;
                            const EnsArgs e = adjoint_args(n, 1ull << b, diag != 0, cap);
                            if (e.part_bits >= 1 && static_cast<uint64_t>(ens_grid(e, cap)) < e.units)
                                out += std::to_string(n) + ":" + std::to_string(b) + ":" + std::to_string(cap) + (diag ? ":diag " : ":flip ");
                        }
            std::printf("%s\n", out.empty() ? "none" : out.c_str());
            continue;
        }
        if (what != "case") {
            std::printf("?\n");
            continue;
        }
        int n, b, pivot, cap;
        in >> n >> b >> pivot >> cap;
        const bool diag = pivot < 0;
        const EnsArgs e = adjoint_args(n, 1ull << b, diag, cap);
        const Walk w = walk(e, n, diag, pivot);
        std::printf("%d %d %d %" PRIu64 " %d %d | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", e.item_bits,
                    e.part_bits, e.share_bits, e.units, ens_grid(e, cap), wave_in_one_member(e) ? 1 : 0, w.checked, w.cover_min, w.cover_max, w.bad_owner,
                    w.bad_member, w.bad_table, w.bad_partial, w.bad_fit);
    }
    return 0;
}

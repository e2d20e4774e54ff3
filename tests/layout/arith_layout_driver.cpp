// TEST INFRASTRUCTURE: text front end of csrc/qsv_arith_layout.h (the host side of qsv_apply_arith), driven by
// tests/test_arith_layout_host.py under AddressSanitizer + UBSan.  One request per line, one answer per line:
//   seg <count> <bit> x count                  -> <n_seg> (<pos> <j> <len>) x n_seg        bits: most significant value bit first
//   form <n> <lowest operand bit>              -> <form>          the lowest bit among target, source and controls
//   shape <n> <used> <max_items_log2>          -> <form> <items_log2> <item_bit0> <item_bit1> <W> <grid> <block>
//   triples <k> (<M> <a> <y>) x k              -> <reciprocal(M)> <reduce(a y, M)> per triple
//   inv <a> <M>                                -> <mod_inverse>
//   tinv <len> <entry> x len                   -> 1 <inverse entries> | 0
//   create <kind> <m> <mx> <a> <c> <modulus> <has_table> <len> <entry> x len
//        -> refused: <message> | ok <M> <pow2> <recip> then for the map's own gather and its inverse's:
//           <body> <a> <c> <identity> <table len> <entries>
//   gather <create's arguments> <inverse> <n> <max_items_log2> <tbits x m> <sbits x mx> <n_controls> <cbits>
//        -> 2^n numbers: the index every destination index is read from, walked exactly as k_arith walks (work items, item
//           bits, arith_source); exit code 3 if a destination is written twice or never, or an index leaves the register
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_arith_layout.h"

using namespace qsv_arith_layout;

static bool read_create(std::istringstream &in, Params *p, const char **refused) {
    int kind, m, mx, has_table;
    uint64_t a, c, modulus, len;
    if (!(in >> kind >> m >> mx >> a >> c >> modulus >> has_table >> len)) return false;
    std::vector<uint64_t> table(len);
    for (uint64_t &v : table)
        if (!(in >> v)) return false;
    *refused = make_params(kind, m, mx, a, c, modulus, has_table ? table.data() : nullptr, len, p);
    return true;
}

static uint64_t source_of(const Set &set, bool pow2, uint64_t i, const ArithArgs &g) {
    const uint32_t *table = set.table.empty() ? nullptr : set.table.data();
    switch (set.body) {
        case BODY_SHIFT: return pow2 ? arith_source<BODY_SHIFT, true>(i, g, table) : arith_source<BODY_SHIFT, false>(i, g, table);
        case BODY_MULT: return pow2 ? arith_source<BODY_MULT, true>(i, g, table) : arith_source<BODY_MULT, false>(i, g, table);
        case BODY_XOR: return arith_source<BODY_XOR, true>(i, g, table);
        default: return arith_source<BODY_TABLE, true>(i, g, table);
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        if (what == "seg") {
            int count;
            if (!(in >> count)) return 2;
            std::vector<int> bits(count);
            for (int &b : bits)
                if (!(in >> b)) return 2;
            const std::vector<uint32_t> segs = segments(bits.data(), count);
            std::printf("%zu", segs.size());
            for (uint32_t s : segs) std::printf(" %u %u %u", seg_pos(s), seg_j(s), seg_len(s));
            // extract and scatter undo each other on the operand's bits
            uint64_t mask = 0;
            for (int b : bits) mask |= 1ull << b;
            const uint64_t probe = 0xa5a5a5a5a5a5a5a5ull & mask;
            if (scatter(extract(probe, segs.data(), static_cast<int>(segs.size())), segs.data(), static_cast<int>(segs.size())) != probe) return 3;
            std::printf("\n");
        } else if (what == "form") {
            int n, t0;
            if (!(in >> n >> t0)) return 2;
            std::printf("%d\n", choose_form(n, t0));
        } else if (what == "shape") {
            int n, max_items;
            uint64_t used;
            if (!(in >> n >> used >> max_items)) return 2;
            const Shape s = launch_shape(n, used, max_items);
            std::printf("%d %d %d %d %" PRIu64 " %u %d\n", s.form, s.items_log2, s.item_bit[0], s.item_bit[1], s.W, s.grid, ARITH_BLOCK);
        } else if (what == "triples") {
            size_t k;
            if (!(in >> k)) return 2;
            for (size_t t = 0; t < k; ++t) {
                uint64_t M, a, y;
                if (!(in >> M >> a >> y)) return 2;
                const uint64_t R = reciprocal(M);
                std::printf("%s%" PRIu64 " %" PRIu64, t ? " " : "", R, reduce(a * y, M, R));
            }
            std::printf("\n");
        } else if (what == "inv") {
            uint64_t a, M;
            if (!(in >> a >> M)) return 2;
            std::printf("%" PRIu64 "\n", mod_inverse(a, M));
        } else if (what == "tinv") {
            size_t len;
            if (!(in >> len)) return 2;
            std::vector<uint32_t> table(len), inv;
            for (uint32_t &v : table)
                if (!(in >> v)) return 2;
            if (!invert_table(table, &inv)) {
                std::printf("0\n");
                continue;
            }
            std::printf("1");
            for (uint32_t v : inv) std::printf(" %u", v);
            std::printf("\n");
        } else if (what == "create") {
            Params p;
            const char *refused = nullptr;
            if (!read_create(in, &p, &refused)) return 2;
            if (refused) {
                std::printf("refused: %s\n", refused);
                continue;
            }
            std::printf("ok %" PRIu64 " %d %" PRIu64, p.M, p.pow2 ? 1 : 0, p.recip);
            // gather_inv is the map itself read as a gather, gather_fwd its inverse
            for (const Set *s : {&p.gather_inv, &p.gather_fwd}) {
                std::printf(" %d %" PRIu64 " %" PRIu64 " %d %zu", s->body, s->a, s->c, s->identity ? 1 : 0, s->table.size());
                for (uint32_t v : s->table) std::printf(" %u", v);
            }
            std::printf("\n");
        } else if (what == "gather") {
            Params p;
            const char *refused = nullptr;
            if (!read_create(in, &p, &refused) || refused) return 2;
            int inverse, n, max_items, n_controls;
            if (!(in >> inverse >> n >> max_items) || n > 20) return 2;
            std::vector<int> tbits(p.m), sbits(p.mx);
            for (int &b : tbits)
                if (!(in >> b)) return 2;
            for (int &b : sbits)
                if (!(in >> b)) return 2;
            if (!(in >> n_controls)) return 2;
            std::vector<int> cbits(n_controls);
            for (int &b : cbits)
                if (!(in >> b)) return 2;
            const Set &set = inverse ? p.gather_inv : p.gather_fwd;
            const Shape shape = launch_shape(n, used_mask(p.m, tbits.data(), p.mx, sbits.data(), n_controls, cbits.data()), max_items);
            const ArithArgs g = make_args(p, set, shape, tbits.data(), sbits.data(), n_controls, cbits.data());
            const uint64_t amps = 1ull << n;
            std::vector<uint64_t> from(amps, ~0ull);
            for (uint64_t w = 0; w < g.W; ++w) {
                const uint64_t to = arith_base(w, g), src = source_of(set, p.pow2, to, g);
                for (int u = 0; u < (1 << g.items_log2); ++u) {
                    uint64_t off = 0;
                    for (int k = 0; k < g.items_log2; ++k)
                        if ((u >> k) & 1) off |= 1ull << g.item_bit[k];
                    if ((to | off) >= amps || (src | off) >= amps || from[to | off] != ~0ull) return 3;
                    from[to | off] = src | off;
                }
            }
            for (uint64_t i = 0; i < amps; ++i) {
                if (from[i] == ~0ull) return 3;
                std::printf("%s%" PRIu64, i ? " " : "", from[i]);
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}

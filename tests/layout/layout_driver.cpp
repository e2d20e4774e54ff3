// TEST INFRASTRUCTURE: prints what qsv_layout.h and qsv_readout_layout.h compute for requests read from stdin
// (tests/test_layout_host.py, tests/test_readout_layout_host.py).
//
// One request per input line, one answer line per request; numbers are decimal integers, doubles are printed as %a.
//   split n k bits..                         -> enough KB | high.. | low.. | standin..
//   order n k transposed a_in_place bits..   -> kernel_bits.. | address_bits.. | inserted_bits..
//   offsets nb addr_bit..                    -> off[0 .. 2^nb)
//   ui k bits.. kernel_bit..                 -> ui[0 .. 2^k)
//   matrix layout D rows ui.. m_user..       -> the doubles written (m_user: 2 D D doubles)
//   enum W or_mask nins inserted..           -> W or_mask nins pos..
//   low n k bits..                           -> amask bmask na | abit.. | aE.. | bdep[0..8)
//   seq arity j0 j1 m..                      -> code m[0..32)
//   takes n k nctrl bits.. cbits..           -> 0 / 1
//   tilecut n k ngates bits.. {arity leg0 leg1 m..}..  -> status | tile_bits.. | passes {first count q0..q3}.. | {code m[0..32)}..
//   limits                                   -> DISPATCH_TILES DISPATCH_ITEMS TILE_SEQ_MAX_PASSES
//   ranges W limit                           -> {w0 count}..
//   launch12 KH KL sub W unroll remap ubit cap hbit0 hbit1  -> U ubit remap grid   (KH < 0: the diagonal launch, k_diag)
//   form n k real variant complex_product mtile bits..  -> form transposed realm m3
//   pass n tile_high count {kind k b0 b1 nctrl cbits.. m[0..32)}..
//                                            -> status | tile_bits.. | groups {first count q0..q3 gates}.. | {form code rc tc tz0 tz1 omask m[0..32)}..
// qsv_readout_layout.h:
//   permute n src_bit_of_dst_bit..           -> tiles bytes | tile_dst[0..6) | tile_src[0..6) | lut[0 .. 256 bytes)
//   rdm n amps k variant remap cus bits..    -> big old_form T P S blocks entries | sorted.. | off[0 .. 16 T) |
//                                               W nins D pos[0..8) | tiles nins k l h lmask log_s regions pos[0..8) | hoff[0..64)
//   rdmunpack n amps k variant remap cus bits.. raw[0 .. entries)  -> rho_out[0 .. 2 D D)
//   sample chunks shots sums.. u..           -> status total | chunk.. | resid..
//   samplewalk threads slots residual p..    -> offset in the chunk   (p: threads * slots doubles)
//   paulisum n terms {xmask zmask}..         -> per pass of qsv_pauli_plan::plan: ok width items xmask pivot odd zmask[0..8) |
//   passraw n xmask pivot count {zmask n_y}..  -> ok width            (a pass as given, well-formed or not)
//   paulirot n terms {xmask zmask cs sn}..   -> per pass of qsv_pauli_rotation_plan::plan:
//                                               ok width items xmask pivot diag rot zmask[0..8) cs[0..8) sn[0..8) |
//   rotraw n xmask pivot count {term_xmask zmask n_y}..  -> ok width  (index = 0 .. count-1, cs = 0.5, sn = 0.25)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qsv_layout.h"
#include "qsv_readout_layout.h"

using namespace qsv_layout;
using namespace qsv_readout_layout;

static std::vector<int> ints(std::istream &in, int count) {
    std::vector<int> v(count > 0 ? count : 0);
    for (int &x : v) in >> x;
    return v;
}
static std::vector<double> doubles(std::istream &in, size_t count) {
    std::vector<double> v(count);
    for (double &x : v) in >> x;
    return v;
}
template <class V>
static void put_ints(const V &v) {
    for (auto x : v) std::printf(" %lld", static_cast<long long>(x));
}
static void put_doubles(const double *m, size_t count) {
    for (size_t i = 0; i < count; ++i) std::printf(" %a", m[i]);
}
static unsigned long long u64(std::istream &in) {
    unsigned long long v = 0;
    in >> v;
    return v;
}
static RdmPlan read_rdm_plan(std::istream &in, std::vector<int> &bits) {
    int n, k, variant, remap, cus;
    in >> n;
    const unsigned long long amps = u64(in);
    in >> k >> variant >> remap >> cus;
    if (k < 1 || k > MAX_K || k > n) std::exit(3);
    bits = ints(in, k);
    return rdm_plan(n, amps, k, bits.data(), variant, remap, cus);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "split" || what == "low") {
            int n, k;
            in >> n >> k;
            const std::vector<int> bits = ints(in, k);
            const Split s = split_targets(k, bits.data(), n);
            if (what == "split") {
                std::printf("%d %d |", s.enough ? 1 : 0, s.KB);
                put_ints(s.high);
                std::printf(" |");
                put_ints(s.low);
                std::printf(" |");
                put_ints(s.standin);
            } else {
                if (!s.enough) return 3;
                const LowFields f = low_fields(s);
                LdsArgs g = with_enumeration<LdsArgs>(enumeration(1, inserted_bits(s)));
                set_low_fields(g, f);
                std::printf("%u %u %d |", g.amask, g.bmask, g.na);
                put_ints(std::vector<int>(g.abit, g.abit + g.na));
                std::printf(" |");
                put_ints(std::vector<int>(g.aE, g.aE + g.na));
                std::printf(" |");
                put_ints(std::vector<uint32_t>(g.bdep, g.bdep + 8));
            }
        } else if (what == "order") {
            int n, k, transposed, a_in_place;
            in >> n >> k >> transposed >> a_in_place;
            const std::vector<int> bits = ints(in, k);
            const Split s = transposed ? split_targets(k, bits.data(), n) : untransposed(k, bits.data());
            if (!s.enough) return 3;
            put_ints(kernel_bits(s));
            std::printf(" |");
            put_ints(address_bits(s, a_in_place != 0));
            std::printf(" |");
            put_ints(inserted_bits(s));
        } else if (what == "offsets") {
            int nb;
            in >> nb;
            put_ints(offsets(ints(in, nb)));
        } else if (what == "ui") {
            int k;
            in >> k;
            const std::vector<int> bits = ints(in, k), kb = ints(in, k);
            put_ints(user_index(k, bits.data(), kb.data()));
        } else if (what == "matrix") {
            int layout, D, rows;
            in >> layout >> D >> rows;
            const std::vector<int> ui = ints(in, D);
            const std::vector<double> m_user = doubles(in, 2ull * D * D);
            const std::vector<double> m = matrix(static_cast<MatrixLayout>(layout), D, m_user.data(), ui.data(), rows);
            std::printf("%d", is_real(D, m_user.data()) ? 1 : 0);
            put_doubles(m.data(), m.size());
        } else if (what == "enum") {
            unsigned long long W, or_mask;
            int nins;
            in >> W >> or_mask >> nins;
            const BigArgs g = with_enumeration<BigArgs>(enumeration(W, ints(in, nins), or_mask));
            std::printf("%llu %llu %d", static_cast<unsigned long long>(g.W), static_cast<unsigned long long>(g.or_mask), g.nins);
            put_ints(std::vector<uint32_t>(g.pos, g.pos + g.nins));
        } else if (what == "seq") {
            int arity, j0, j1;
            in >> arity >> j0 >> j1;
            const std::vector<double> m = doubles(in, arity == 1 ? 8 : 32);
            const SeqGate r = seq_record(arity, j0, j1, m.data());
            std::printf("%d", r.code);
            put_doubles(r.m, 32);
        } else if (what == "takes") {
            int n, k, nctrl;
            in >> n >> k >> nctrl;
            const std::vector<int> bits = ints(in, k), cbits = ints(in, nctrl);
            std::printf("%d", tile12_takes(1ull << n, k, bits.data(), nctrl, cbits.data()) ? 1 : 0);
        } else if (what == "tilecut") {
            int n, k, ngates;
            in >> n >> k >> ngates;
            const std::vector<int> bits = ints(in, k);
            std::vector<int> arity(ngates), legs(2 * ngates);
            std::vector<double> mats;
            for (int g = 0; g < ngates; ++g) {
                in >> arity[g] >> legs[2 * g] >> legs[2 * g + 1];
                const std::vector<double> m = doubles(in, arity[g] == 1 ? 8 : 32);
                mats.insert(mats.end(), m.begin(), m.end());
            }
            const TileCut cut = cut_tile_passes(n, k, bits.data(), ngates, arity.data(), legs.data(), mats.data());
            std::printf("%d |", static_cast<int>(cut.status));
            if (cut.status == TileCut::OK) {
                put_ints(cut.tile_bits);
                std::printf(" | %zu", cut.passes.size());
                for (const TilePass &p : cut.passes) std::printf(" %d %d %d %d %d %d", p.first, p.count, p.q[0], p.q[1], p.q[2], p.q[3]);
                std::printf(" |");
                for (const SeqGate &r : cut.rec) {
                    std::printf(" %d", r.code);
                    put_doubles(r.m, 32);
                }
            }
        } else if (what == "limits") {
            std::printf("%llu %llu %d", static_cast<unsigned long long>(DISPATCH_TILES),
                        static_cast<unsigned long long>(DISPATCH_ITEMS), TILE_SEQ_MAX_PASSES);
        } else if (what == "ranges") {
            unsigned long long W, limit;
            in >> W >> limit;
            for (const Range &r : dispatch_ranges(W, limit))
                std::printf(" %llu %llu", static_cast<unsigned long long>(r.w0), static_cast<unsigned long long>(r.count));
        } else if (what == "launch12") {
            int KH, KL, sub, hbit[2];
            LaunchOptions o;
            in >> KH >> KL >> sub;
            const unsigned long long W = u64(in);
            in >> o.unroll >> o.remap >> o.ubit >> o.grid_cap >> hbit[0] >> hbit[1];
            if (KH > 2) return 3;
            const Launch12 l = KH < 0 ? diag_launch(sub != 0, W, o) : dense_launch(KH, KL, hbit, sub != 0, W, o);
            std::printf("%d %d %d %d", l.U, l.ubit, l.remap, l.grid);
        } else if (what == "form") {
            int n, k, real, variant, cp, mtile;
            in >> n >> k >> real >> variant >> cp >> mtile;
            const std::vector<int> bits = ints(in, k);
            const FormChoice f = choose_form(n, 1ull << n, k, bits.data(), real != 0, FormOptions{variant, cp, mtile != 0});
            std::printf("%d %d %d %d", static_cast<int>(f.form), f.transposed ? 1 : 0, f.realm ? 1 : 0, f.m3 ? 1 : 0);
        } else if (what == "pass") {
            int n, count;
            unsigned long long tile_high;
            in >> n >> tile_high >> count;
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
                put_ints(std::vector<int>(pr.tile_bits, pr.tile_bits + qsv_plan::TILE_BITS));
                std::printf(" | %zu", pr.grp.size());
                for (const PassGroup &g : pr.grp)
                    std::printf(" %d %d %d %d %d %d %llu", g.first, g.count, g.q[0], g.q[1], g.q[2], g.q[3], static_cast<unsigned long long>(g.gates));
                std::printf(" |");
                for (const PassGate &g : pr.rec) {
                    std::printf(" %d %d %u %u %d %d %llu", g.form, g.code, g.rc, g.tc, g.tz0, g.tz1, static_cast<unsigned long long>(g.omask));
                    put_doubles(g.m, 32);
                }
            }
        } else if (what == "permute") {
            int n;
            in >> n;
            const std::vector<int> order = ints(in, n);
            const PermTile t = permute_tile(n, order.data());
            std::printf("%llu %d |", static_cast<unsigned long long>(t.args.tiles), t.args.bytes);
            put_ints(std::vector<int>(t.args.tile_dst, t.args.tile_dst + 6));
            std::printf(" |");
            put_ints(std::vector<int>(t.args.tile_src, t.args.tile_src + 6));
            std::printf(" |");
            put_ints(t.lut);
        } else if (what == "rdm") {
            std::vector<int> bits;
            const RdmPlan p = read_rdm_plan(in, bits);
            std::printf("%d %d %d %d %d %d %d |", p.big ? 1 : 0, p.old_form ? 1 : 0, p.T, p.P, p.S, p.blocks, p.entries);
            put_ints(p.sorted);
            std::printf(" |");
            put_ints(p.off);
            std::printf(" | %llu %d %d", static_cast<unsigned long long>(p.g.W), p.g.nins, p.g.D);
            put_ints(std::vector<uint32_t>(p.g.pos, p.g.pos + 8));
            std::printf(" | %llu %d %d %d %d %u %d %u", static_cast<unsigned long long>(p.gt.tiles), p.gt.nins, p.gt.k, p.gt.l, p.gt.h,
                        p.gt.lmask, p.gt.log_s, p.gt.regions);
            put_ints(std::vector<uint32_t>(p.gt.pos, p.gt.pos + 8));
            std::printf(" |");
            put_ints(std::vector<uint64_t>(p.gt.hoff, p.gt.hoff + 64));
        } else if (what == "rdmunpack") {
            std::vector<int> bits;
            const RdmPlan p = read_rdm_plan(in, bits);
            const std::vector<double> raw = doubles(in, p.entries);
            std::vector<double> rho(2ull * p.D * p.D);
            rdm_unpack(p, bits.data(), raw.data(), rho.data());
            put_doubles(rho.data(), rho.size());
        } else if (what == "sample") {
            int chunks, shots;
            in >> chunks >> shots;
            const std::vector<double> sums = doubles(in, chunks), u = doubles(in, shots);
            const SampleChunks c = sample_chunks(sums, u.data(), shots);
            std::printf("%d %a |", static_cast<int>(c.status), c.total);
            if (c.status == SampleChunks::OK) {
                put_ints(c.chunk);
                std::printf(" |");
                put_doubles(c.resid.data(), c.resid.size());
            }
        } else if (what == "samplewalk") {
            int threads, slots;
            double residual;
            in >> threads >> slots >> residual;
            if (threads < 1 || slots < 1) std::exit(3);
            const std::vector<double> p = doubles(in, static_cast<size_t>(threads) * slots);
            std::printf("%d", sample_walk(p.data(), threads, slots, residual));
        } else if (what == "paulisum") {
            int n, count;
            in >> n >> count;
            std::vector<qsv_pauli_plan::Term> terms(count);
            for (auto &t : terms) t.xmask = u64(in), t.zmask = u64(in);
            for (const qsv_pauli_plan::Pass &pass : qsv_pauli_plan::plan(terms)) {
                const PauliPass a = pauli_pass_args(pass, 1ull << n);
                std::printf(" %d %d %llu %llu %d %u", a.ok ? 1 : 0, a.width, static_cast<unsigned long long>(a.g.items),
                            static_cast<unsigned long long>(a.g.xmask), a.g.pivot, a.g.odd);
                put_ints(std::vector<uint64_t>(a.g.zmask, a.g.zmask + qsv_pauli_plan::PAULI_TERMS_PER_PASS));
                std::printf(" |");
            }
        } else if (what == "passraw") {
            int n, count;
            qsv_pauli_plan::Pass pass;
            in >> n;
            pass.xmask = u64(in);
            in >> pass.pivot >> count;
            for (int t = 0; t < count; ++t) {
                pass.zmask.push_back(u64(in));
                pass.n_y.push_back(ints(in, 1)[0]);
                pass.index.push_back(t);
            }
            const PauliPass a = pauli_pass_args(pass, 1ull << n);
            std::printf("%d %d", a.ok ? 1 : 0, a.width);
        } else if (what == "paulirot") {
            int n, count;
            in >> n >> count;
            std::vector<qsv_pauli_plan::Term> terms(count);
            std::vector<double> cs(count), sn(count);
            for (int t = 0; t < count; ++t) {
                terms[t].xmask = u64(in), terms[t].zmask = u64(in);
                in >> cs[t] >> sn[t];
            }
            constexpr int CAP = qsv_pauli_rotation_plan::ROTATIONS_PER_PASS;
            for (const qsv_pauli_rotation_plan::Pass &pass : qsv_pauli_rotation_plan::plan(terms)) {
                const PauliRotate a = pauli_rotate_args(pass, 1ull << n, cs.data(), sn.data());
                std::printf(" %d %d %llu %llu %d %u %u", a.ok ? 1 : 0, a.width, static_cast<unsigned long long>(a.g.items),
                            static_cast<unsigned long long>(a.g.xmask), a.g.pivot, a.g.diag, a.g.rot);
                put_ints(std::vector<uint64_t>(a.g.zmask, a.g.zmask + CAP));
                put_doubles(a.g.cs, CAP);
                put_doubles(a.g.sn, CAP);
                std::printf(" |");
            }
        } else if (what == "rotraw") {
            int n, count;
            qsv_pauli_rotation_plan::Pass pass;
            in >> n;
            pass.xmask = u64(in);
            in >> pass.pivot >> count;
            for (int t = 0; t < count; ++t) {
                pass.term_xmask.push_back(u64(in));
                pass.zmask.push_back(u64(in));
                pass.n_y.push_back(ints(in, 1)[0]);
                pass.index.push_back(t);
            }
            const std::vector<double> cs(count + 1, 0.5), sn(count + 1, 0.25);
            const PauliRotate a = pauli_rotate_args(pass, 1ull << n, cs.data(), sn.data());
            std::printf("%d %d", a.ok ? 1 : 0, a.width);
        } else {
            return 2;
        }
        if (!in && !in.eof()) return 2;
        std::printf("\n");
    }
    std::fflush(stdout);
    return 0;
}

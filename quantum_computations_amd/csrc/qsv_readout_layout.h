// Host-side layouts of the read-out and Pauli launchers (qsv_readout.hip, qsv_pauli.hip): plain C++, no HIP, so that the
// host tests can compile it alone (tests/test_readout_layout_host.py).
//
// A launcher asks this header for the argument struct and tables of its kernel, ensures or stages buffers, launches and
// copies back.  Everything here is index arithmetic; the index spaces are those of qsv_layout.h.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "qsv_layout.h"
#include "qsv_pauli_plan.h"
#include "qsv_pauli_rotation_plan.h"

namespace qsv_readout_layout {

constexpr int RO_MIN_QUBITS = 14;  // below this the plain grid-stride forms run (tiles of 2^10 amplitudes must divide)

// ---- argument types of the kernels (passed by value: field order and sizes are ABI) -------------------------------------

// k_permute
struct PermArgs {
    int32_t n;
    uint8_t src_bit[64];  // bit j of the destination index comes from bit src_bit[j] of the source index
};
static_assert(sizeof(PermArgs) == 68, "kernel argument layout");

// k_permute_s
struct PermTileArgs {
    uint64_t tiles;          // amps / 64
    int32_t bytes;           // ceil(n / 8): lookup tables
    uint8_t tile_dst[6];     // destination bit of lane bit k, ascending (tile_dst[0..2] = 0, 1, 2)
    uint8_t tile_src[6];     // source bit that feeds it
};
static_assert(sizeof(PermTileArgs) == 24, "kernel argument layout");

// k_rdm, k_rdm_small
struct RdmArgs {
    uint64_t W;          // groups = amps >> k
    uint64_t or_mask;    // unused (0); lets deposit() serve this struct too
    int32_t nins;        // k
    int32_t D;           // 2^k
    uint32_t pos[8];     // ascending kept bits
};
static_assert(sizeof(RdmArgs) == 56, "kernel argument layout");
constexpr int RDM_LOADS = 4;   // k_rdm: 16-byte loads per lane and buffer, RDM_LOADS / T quads of groups

// k_rdm_tile
struct RdmTileArgs {
    uint64_t tiles;      // tiles of 64 S groups
    uint64_t or_mask;    // unused (0); lets deposit() serve this struct too
    int32_t nins;        // h: kept bits >= 6
    uint32_t pos[8];     // those bits, ascending
    int32_t k, l, h;     // kept bits, of which below / from bit 6
    uint32_t lmask;      // lane bits that are kept bits
    int32_t log_s;       // 2^k < 16: log2 of the groups sharing the 16 rows
    uint32_t regions;    // tile order: R > 1 walks R contiguous regions of the register side by side
    uint64_t hoff[64];   // offset of setting c_h of the kept bits >= 6 (kernel arguments: scalar loads, no upload)
};
static_assert(sizeof(RdmTileArgs) == 80 + 64 * 8, "kernel argument layout");

// One planned pass of qsv_expect_pauli_sum (qsv_pauli_plan.h): up to T Pauli strings with one shared xmask.
struct PauliPassArgs {
    uint64_t items;      // pairs (amps / 2), or amps for the diagonal group
    uint64_t xmask;
    int32_t pivot;       // lowest set bit of xmask (unused by the diagonal form)
    uint32_t odd;        // bit t: term t has odd nY and accumulates Im c instead of Re c
    uint64_t zmask[qsv_pauli_plan::PAULI_TERMS_PER_PASS];   // 0 beyond the pass's terms
};
static_assert(sizeof(PauliPassArgs) == 24 + 8 * qsv_pauli_plan::PAULI_TERMS_PER_PASS, "kernel argument layout");

// One planned pass of qsv_apply_pauli_rotations (qsv_pauli_rotation_plan.h): up to T rotations exp(-i theta/2 P), each
// diagonal or flipping the pass's xmask, applied in the caller's order to every pair {i, i ^ xmask}.
struct PauliRotateArgs {
    uint64_t items;      // pairs (amps / 2), or amps for a diagonal pass
    uint64_t xmask;
    int32_t pivot;       // highest set bit of xmask (unused by the diagonal form)
    uint32_t diag;       // bit t: term t is diagonal (set beyond the pass's terms, which are padded with theta = 0)
    uint32_t rot;        // bits 2t, 2t + 1: nY & 3 of term t
    uint64_t zmask[qsv_pauli_rotation_plan::ROTATIONS_PER_PASS];
    double cs[qsv_pauli_rotation_plan::ROTATIONS_PER_PASS];   // cos(theta / 2), computed on the host in double precision
    double sn[qsv_pauli_rotation_plan::ROTATIONS_PER_PASS];   // sin(theta / 2)
};
static_assert(sizeof(PauliRotateArgs) == 32 + 24 * qsv_pauli_rotation_plan::ROTATIONS_PER_PASS, "kernel argument layout");

// One planned pass of qsv_apply_pauli_sum (qsv_pauli_plan.h): dst (+)= (sum_t c_t P_t) src for up to T Pauli strings with
// one shared xmask.  (P x)[k] = i^{nY} s(k ^ xmask) x[k ^ xmask]: with d_t = c_t i^{nY_t} the pair {i, j = i ^ xmask} gets
// dst[i] (+)= f_i src[j], f_i = sum_t d_t s_t(j), and dst[j] (+)= f_j src[i], f_j = sum_t d_t s_t(i).
struct PauliSumApplyArgs {
    uint64_t items;      // pairs (amps / 2), or amps for the diagonal group
    uint64_t xmask;
    int32_t pivot;       // highest set bit of xmask: the pass writes (unused by the diagonal form)
    uint32_t odd;        // bit t: term t has odd nY, s_t(j) = -s_t(i)
    uint64_t zmask[qsv_pauli_plan::PAULI_TERMS_PER_PASS];   // 0 beyond the pass's terms
    double d_re[qsv_pauli_plan::PAULI_TERMS_PER_PASS];      // d_t = c_t i^{nY_t}, 0 beyond the pass's terms
    double d_im[qsv_pauli_plan::PAULI_TERMS_PER_PASS];
};
static_assert(sizeof(PauliSumApplyArgs) == 24 + 24 * qsv_pauli_plan::PAULI_TERMS_PER_PASS, "kernel argument layout");

// ---- qubit permutation (k_permute_s) ------------------------------------------------------------------------------------
struct PermTile {
    PermTileArgs args;
    std::vector<uint64_t> lut;   // [bytes][256]
};
inline PermTile permute_tile(int n, const int *src_bit_of_dst_bit) {
    PermTile out;
    PermTileArgs &t = out.args;
    memset(&t, 0, sizeof(t));
    t.tiles = (1ull << n) >> 6;
    t.bytes = (n + 7) / 8;
    // the tile: destination bits 0..2, the destinations of source bits 0..2, then the lowest other bits up to six
    std::vector<int> tile = {0, 1, 2};
    for (int j = 3; j < n; ++j)
        if (src_bit_of_dst_bit[j] < 3) tile.push_back(j);
    for (int j = 3; j < n && tile.size() < 6; ++j)
        if (std::find(tile.begin(), tile.end(), j) == tile.end()) tile.push_back(j);
    std::sort(tile.begin(), tile.end());
    for (int k = 0; k < 6; ++k) {
        t.tile_dst[k] = static_cast<uint8_t>(tile[k]);
        t.tile_src[k] = static_cast<uint8_t>(src_bit_of_dst_bit[tile[k]]);
    }
    // lut[b][v]: where the destination-index bits 8b .. 8b+7 (value v) come from in the source index
    out.lut.assign(static_cast<size_t>(t.bytes) * 256, 0);
    for (int b = 0; b < t.bytes; ++b)
        for (int v = 0; v < 256; ++v)
            for (int i = 0; i < 8 && 8 * b + i < n; ++i)
                if ((v >> i) & 1) out.lut[b * 256 + v] |= 1ull << src_bit_of_dst_bit[8 * b + i];
    return out;
}

// ---- reduced density matrix (k_rdm_tile, k_rdm, k_rdm_small) ------------------------------------------------------------
// Everything qsvk_reduced_density works out before it touches the device.  k = 1..6 kept bits; `remap` is QSV_OPT_REMAP
// (-1: the form's own tile order), `cus` the device's compute units.
struct RdmPlan {
    int k = 0, D = 0;
    std::vector<int> sorted;     // the kept bits, ascending: kernel row bit i <-> sorted[i]
    int T = 0, P = 0, S = 0;     // row tiles of 16, tile pairs ti <= tj, groups sharing a 16-row tile (2^k < 16)
    bool big = false;            // a matrix-core form (else k_rdm_small)
    bool old_form = false;       // round 2's per-lane row loads, k_rdm (measurement variant 2)
    std::vector<uint64_t> off;   // [16 T] row offsets (k_rdm, k_rdm_small)
    RdmArgs g;
    RdmTileArgs gt;              // filled for the tile form only
    int blocks = 0;              // workgroups of the matrix-core forms = partial results
    int entries = 0;             // doubles of one result
};
inline RdmPlan rdm_plan(int n, uint64_t amps, int k, const int *bits, int readout_variant, int remap, int cus) {
    RdmPlan p;
    p.k = k;
    const int D = p.D = 1 << k;
    p.sorted.assign(bits, bits + k);
    std::sort(p.sorted.begin(), p.sorted.end());
    const std::vector<int> &sorted = p.sorted;
    const int T = p.T = D <= 16 ? 1 : D <= 32 ? 2 : 4;
    p.P = T * (T + 1) / 2;
    p.off.assign(16 * T, 0);
    for (int r = 0; r < D; ++r)
        for (int i = 0; i < k; ++i)
            if ((r >> i) & 1) p.off[r] |= 1ull << sorted[i];
    RdmArgs &g = p.g;
    memset(&g, 0, sizeof(g));
    g.W = amps >> k;
    g.nins = k;
    g.D = D;
    for (int i = 0; i < k; ++i) g.pos[i] = static_cast<uint32_t>(sorted[i]);
    const int S = p.S = D < 16 ? 16 / D : 1;
    p.old_form = readout_variant == 2;
    p.big = n >= RO_MIN_QUBITS && (p.old_form ? g.W % (4ull * S * 4 * (RDM_LOADS / T)) == 0           // whole iterations
                                              : g.W % (64ull * S) == 0 && g.W >= 64ull * S);          // whole tiles
    RdmTileArgs &gt = p.gt;
    memset(&gt, 0, sizeof(gt));
    if (p.big && !p.old_form) {
        gt.k = k;
        for (int i = 0; i < k; ++i) {
            if (sorted[i] < 6) {
                gt.lmask |= 1u << sorted[i];
                ++gt.l;
            } else {
                gt.pos[gt.h++] = static_cast<uint32_t>(sorted[i]);
            }
        }
        gt.nins = gt.h;
        gt.log_s = S == 1 ? 0 : S == 2 ? 1 : S == 4 ? 2 : 3;
        gt.tiles = g.W / (64ull * S);
        for (int c = 0; c < (1 << gt.h); ++c)
            for (int j = 0; j < gt.h; ++j)
                if ((c >> j) & 1) gt.hoff[c] |= 1ull << gt.pos[j];
        // 8 regions where a kept bit sits on the high address bits (k <= 4 on bits 24..27: 1.14 -> 0.82 ms at n = 28) and
        // for 64-row tiles; plain order otherwise (within 5 % either way: profiles/r03_rdm.txt)
        const uint32_t want = remap >= 0 ? static_cast<uint32_t>(remap) : ((sorted.back() >= 20 || k == 6) ? 8u : 0u);
        gt.regions = want > 1 && gt.tiles % want == 0 ? want : 0;
    }
    if (p.big && p.old_form) {
        // a power-of-two grid, so that (waves in the grid) x RDM_U divides the (power-of-two) number of steps
        const uint64_t most = std::min<uint64_t>((T <= 2 ? 4ull : 2ull) * cus, std::max<uint64_t>(1, g.W / (4ull * S) / (4 * (RDM_LOADS / T))));
        p.blocks = 1;
        while (2ull * p.blocks <= most) p.blocks *= 2;
    } else if (p.big) {   // persistent workgroups, as many as the LDS tiles (16 T KiB) and the accumulators let a CU hold
        p.blocks = static_cast<int>(std::min<uint64_t>(gt.tiles, static_cast<uint64_t>(T == 4 ? 2 : T == 2 ? 4 : 8) * cus));
    }
    p.entries = p.big ? p.P * 2 * 256 : 2 * D * D;
    return p;
}

// raw (plan.entries doubles, as the kernels leave them) -> rho_out: 4^k complex, row-major, row / column index bit
// (k-1-j) <-> bits[j].
inline void rdm_unpack(const RdmPlan &p, const int *bits, const double *raw, double *rho_out) {
    const int D = p.D, T = p.T, S = p.S;
    // kernel order (row bit i <-> sorted[i]) -> caller order (bit k-1-j <-> bits[j])
    const std::vector<int> ui = qsv_layout::user_index(p.k, bits, p.sorted.data());
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            double vr, vi;
            if (p.big) {
                // tile pair p = (ti <= tj); D layout: col = lane & 15, row = (lane >> 4) + 4 reg.  Entries below the
                // diagonal are the conjugates of those above it and the diagonal is real, exactly (the matrix cores
                // sum the two mirror entries of a diagonal tile in different orders: equal up to rounding only)
                const bool upper = r <= c;
                const int rr = upper ? r : c, cc = upper ? c : r;
                const int ti = rr / 16, tj = cc / 16;
                // k_rdm_tile<4> holds pair (0, 3) as the block of (3, 0): read it mirrored, imaginary part negated
                const bool mirrored = !p.old_form && T == 4 && ti == 0 && tj == 3;
                int pidx = 0;
                for (int a = 0; a < ti; ++a) pidx += T - a;
                pidx += tj - ti;
                vr = vi = 0.0;
                for (int sgrp = 0; sgrp < S; ++sgrp) {   // 2^k < 16: the diagonal blocks of the shared tile add up
                    int row = rr % 16 + D * sgrp * (D < 16), col = cc % 16 + D * sgrp * (D < 16);
                    if (mirrored) std::swap(row, col);
                    const int reg = row / 4, lane = (row % 4) * 16 + col;
                    vr += raw[((pidx * 2 + 0) * 4 + reg) * 64 + lane];
                    vi += (mirrored ? -1.0 : 1.0) * raw[((pidx * 2 + 1) * 4 + reg) * 64 + lane];
                }
                if (!upper) vi = -vi;  // rho[r][c] = conj(rho[c][r])
                if (r == c) vi = 0.0;
            } else {
                vr = raw[2 * (r * D + c)];
                vi = raw[2 * (r * D + c) + 1];
            }
            const int ur = ui[r], uc = ui[c];
            rho_out[2 * (ur * D + uc)] = vr;
            rho_out[2 * (ur * D + uc) + 1] = vi;
        }
}

// ---- sampling (k_chunk_sums -> here -> k_sample_in_chunk) ---------------------------------------------------------------
// Inverse CDF over the chunk sums: shot s falls into chunk[s] and has resid[s] of probability left to walk inside it.
struct SampleChunks {
    enum Status { OK, ZERO_NORM, DRAW_OUTSIDE /* of [0, 1) */ } status = OK;
    double total = 0.0;
    std::vector<uint64_t> chunk;
    std::vector<double> resid;
};
inline SampleChunks sample_chunks(const std::vector<double> &sums, const double *u, int shots) {
    SampleChunks out;
    const uint64_t chunks = sums.size();
    std::vector<double> cum(chunks + 1, 0.0);
    for (uint64_t c = 0; c < chunks; ++c) cum[c + 1] = cum[c] + sums[c];
    const double total = out.total = cum[chunks];
    if (!(total > 0.0)) return out.status = SampleChunks::ZERO_NORM, out;
    out.chunk.resize(shots);
    out.resid.resize(shots);
    for (int s = 0; s < shots; ++s) {
        if (!(u[s] >= 0.0 && u[s] < 1.0)) return out.status = SampleChunks::DRAW_OUTSIDE, out;
        const double target = u[s] * total;
        uint64_t c = std::upper_bound(cum.begin(), cum.end(), target) - cum.begin();  // first cum > target
        c = c == 0 ? 0 : c - 1;
        while (c + 1 < chunks && sums[c] == 0.0) ++c;  // never land in an empty chunk
        if (c >= chunks) c = chunks - 1;
        out.chunk[s] = c;
        out.resid[s] = target - cum[c];
    }
    return out;
}

// The walk inside the chosen chunk (k_sample_in_chunk spells out the same steps): thread t owns p[t * slots .. (t + 1) * slots),
// the |amp|^2 of its amplitudes, 0 past the end of the register.  Returns the offset in the chunk of the first amplitude
// at which the running sum exceeds `residual` -- over the thread sums first, then over the owner's slots -- and, where
// rounding leaves no such amplitude, of the last one with p > 0: the rule of qsv_channel_layout.h's pick_branch, at both
// levels.  The two levels and pass 1 add the same numbers in different orders, so a residual within rounding of the
// chunk's (or the owner's) sum can find no crossing; an amplitude of weight zero is never the answer (0 if all are zero).
inline int sample_walk(const double *p, int threads, int slots, double residual) {
    double run = 0.0;
    int owner = -1, last = -1;
    for (int t = 0; t < threads; ++t) {
        double s = 0.0;
        for (int k = 0; k < slots; ++k) s += p[t * slots + k];
        if (s > 0.0) last = t;
        if (run + s > residual) {
            owner = t;
            break;
        }
        run += s;
    }
    const bool crossed = owner >= 0;   // `run` is then the sum in front of the owner
    if (!crossed) owner = last < 0 ? 0 : last;
    int slot = -1;
    last = -1;
    for (int k = 0; k < slots; ++k) {
        const double m = p[owner * slots + k];
        if (m > 0.0) last = k;
        if (crossed && run + m > residual) {
            slot = k;
            break;
        }
        run += m;
    }
    if (slot < 0) slot = last < 0 ? 0 : last;
    return owner * slots + slot;
}

// ---- Pauli passes (k_expect_pauli_group, k_pauli_rotate_group) ----------------------------------------------------------
inline int pauli_width(int count) { return count <= 1 ? 1 : count <= 2 ? 2 : count <= 4 ? 4 : 8; }   // the kernels' T

struct PauliPass {
    bool ok = false;     // the pass has 1 .. PAULI_TERMS_PER_PASS terms
    PauliPassArgs g;
    int width = 0;
};
inline PauliPass pauli_pass_args(const qsv_pauli_plan::Pass &p, uint64_t amps) {
    PauliPass out;
    PauliPassArgs &g = out.g;
    memset(&g, 0, sizeof(g));
    const int count = static_cast<int>(p.zmask.size());
    if (count < 1 || count > qsv_pauli_plan::PAULI_TERMS_PER_PASS) return out;
    g.items = p.pivot < 0 ? amps : amps / 2;
    g.xmask = p.xmask;
    g.pivot = p.pivot < 0 ? 0 : p.pivot;
    for (int t = 0; t < count; ++t) {
        g.zmask[t] = p.zmask[t];
        if (p.n_y[t] & 1) g.odd |= 1u << t;
    }
    out.width = pauli_width(count);
    out.ok = true;
    return out;
}

// cs / sn: cos(theta/2) and sin(theta/2) of every term, indexed as the caller's list.
struct PauliRotate {
    bool ok = false;     // 1 .. ROTATIONS_PER_PASS terms, a pivot inside the register that goes with the xmask
    PauliRotateArgs g;
    int width = 0;
};
inline PauliRotate pauli_rotate_args(const qsv_pauli_rotation_plan::Pass &p, uint64_t amps, const double *cs, const double *sn) {
    constexpr int CAP = qsv_pauli_rotation_plan::ROTATIONS_PER_PASS;
    PauliRotate out;
    PauliRotateArgs &g = out.g;
    memset(&g, 0, sizeof(g));
    const int count = static_cast<int>(p.index.size());
    // a pivot at or above the register's top bit: pivot >= n for a register of 2^n amplitudes
    const bool pivot_outside = p.pivot >= 64 || (p.pivot >= 0 && (1ull << p.pivot) >= amps);
    if (count < 1 || count > CAP || pivot_outside || (p.pivot < 0) != (p.xmask == 0) || p.xmask >= amps) return out;
    g.items = p.pivot < 0 ? amps : amps / 2;
    g.xmask = p.xmask;
    g.pivot = p.pivot < 0 ? 0 : p.pivot;
    for (int t = 0; t < CAP; ++t) {
        const bool used = t < count;
        g.zmask[t] = used ? p.zmask[t] : 0;
        g.cs[t] = used ? cs[p.index[t]] : 1.0;
        g.sn[t] = used ? sn[p.index[t]] : 0.0;
        if (!used || p.term_xmask[t] == 0) g.diag |= 1u << t;
        else g.rot |= static_cast<uint32_t>(p.n_y[t] & 3) << (2 * t);
    }
    out.width = pauli_width(count);
    out.ok = true;
    return out;
}

// ---- Pauli sums as operators (k_pauli_sum_apply_group, k_pauli_transition_group, k_pauli_adjoint_group) ------------------
// i^k (re + i im), the factor the kernels leave to the host
inline void times_i_pow(int k, double re, double im, double *out_re, double *out_im) {
    switch (k & 3) {
        case 0: *out_re = re; *out_im = im; break;
        case 1: *out_re = -im; *out_im = re; break;
        case 2: *out_re = -re; *out_im = -im; break;
        default: *out_re = im; *out_im = -re; break;
    }
}

// coeffs: the interleaved complex c_t of every term, indexed as the caller's list.  The planner's own pivot (the lowest
// flipped bit, for passes that only read) is not used: this pass writes and takes the highest, as the rotation pass does.
struct PauliSumApply {
    bool ok = false;     // 1 .. PAULI_TERMS_PER_PASS terms and an xmask inside the register
    PauliSumApplyArgs g;
    int width = 0;
    bool first = false;  // the first pass of a call that overwrites: the old dst is not read
};
inline PauliSumApply pauli_sum_apply_args(const qsv_pauli_plan::Pass &p, uint64_t amps, const double *coeffs, bool first) {
    PauliSumApply out;
    PauliSumApplyArgs &g = out.g;
    memset(&g, 0, sizeof(g));
    const int count = static_cast<int>(p.zmask.size());
    if (count < 1 || count > qsv_pauli_plan::PAULI_TERMS_PER_PASS || p.xmask >= amps) return out;
    g.items = p.xmask ? amps / 2 : amps;
    g.xmask = p.xmask;
    g.pivot = p.xmask ? qsv_pauli_rotation_plan::highest_bit(p.xmask) : 0;
    for (int t = 0; t < count; ++t) {
        g.zmask[t] = p.zmask[t];
        if (p.n_y[t] & 1) g.odd |= 1u << t;
        times_i_pow(p.n_y[t], coeffs[2 * p.index[t]], coeffs[2 * p.index[t] + 1], &g.d_re[t], &g.d_im[t]);
    }
    out.width = pauli_width(count);
    out.first = first;
    out.ok = true;
    return out;
}
// Every pass of a call; `first` is set on pass 0 of a call that does not accumulate, and nowhere else.
inline std::vector<PauliSumApply> pauli_sum_apply_passes(const std::vector<qsv_pauli_plan::Pass> &passes, uint64_t amps,
                                                         const double *coeffs, bool accumulate) {
    std::vector<PauliSumApply> out;
    for (size_t k = 0; k < passes.size(); ++k) out.push_back(pauli_sum_apply_args(passes[k], amps, coeffs, k == 0 && !accumulate));
    return out;
}

// The backward walk of qsv_pauli_rotations_adjoint over one pass of the forward plan: the pass's terms in reverse order,
// each with -theta (cs kept, sn negated); padding as in pauli_rotate_args.  index[t]: the caller's term behind slot t.
struct PauliAdjoint {
    PauliRotate r;
    int index[qsv_pauli_rotation_plan::ROTATIONS_PER_PASS];
    int n_y[qsv_pauli_rotation_plan::ROTATIONS_PER_PASS];    // of the term behind slot t (0: diagonal or padding)
};
inline PauliAdjoint pauli_adjoint_args(const qsv_pauli_rotation_plan::Pass &p, uint64_t amps, const double *cs, const double *sn) {
    qsv_pauli_rotation_plan::Pass back = p;
    std::reverse(back.index.begin(), back.index.end());
    std::reverse(back.term_xmask.begin(), back.term_xmask.end());
    std::reverse(back.zmask.begin(), back.zmask.end());
    std::reverse(back.n_y.begin(), back.n_y.end());
    PauliAdjoint out;
    out.r = pauli_rotate_args(back, amps, cs, sn);
    const int count = out.r.ok ? static_cast<int>(back.index.size()) : 0;
    for (int t = 0; t < qsv_pauli_rotation_plan::ROTATIONS_PER_PASS; ++t) {
        out.index[t] = t < count ? back.index[t] : -1;
        out.n_y[t] = t < count && back.term_xmask[t] ? back.n_y[t] : 0;
        if (t < count) out.r.g.sn[t] = -out.r.g.sn[t];
    }
    return out;
}
// The forward plan's passes in the order the walk takes them: last first.
inline std::vector<PauliAdjoint> pauli_adjoint_passes(const std::vector<qsv_pauli_rotation_plan::Pass> &passes, uint64_t amps,
                                                      const double *cs, const double *sn) {
    std::vector<PauliAdjoint> out;
    for (size_t k = passes.size(); k-- > 0;) out.push_back(pauli_adjoint_args(passes[k], amps, cs, sn));
    return out;
}

}  // namespace qsv_readout_layout
